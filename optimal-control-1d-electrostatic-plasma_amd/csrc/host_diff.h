// host_diff.h -- shared by host_phase.h, host_moments.h, host_pool.h, host_tape.h, host_tangent.h, host_tangent_walk.h, host_head.h,
// host_policy.h and host_actor.h; included by picstep.hip alone, behind its helpers.  The layouts of the carved blocks are
// host_blocks.h's; here: the two functions that allocate one.
#pragma once

static_assert(std::is_same<acc_t, long long>::value, "host_blocks.h: TapeViews::acc is an accumulator row");

// what the layouts read of a handle
inline BlockDims block_dims(const pic_handle* h) {
  BlockDims d;
  d.num_envs = (size_t)h->cfg.num_envs; d.ld = (size_t)h->ld; d.Ng = (size_t)h->cfg.Ng; d.act_modes = (size_t)h->act_modes;
  return d;
}

// The one reserve path of the tape's blocks.  `b` becomes a block laid out by `layout` (size_t(Carver, Views&): host_blocks.h),
// its views go to `views`, and -- with `copy` -- a per-call copy of copy_bytes is allocated with it (keep: b stays as it is, only
// the copy is new).  In this order: size the block; the tape's bytes with it (less what it replaces) against budget_bytes;
// allocate aside; wait for the stream if an old block goes (queued work may still read it); carve; views; bytes.  On any failure
// the tape is as it was, pic_tape_info.bytes included.
template <typename Views, typename Layout>
int tape_reserve(pic_handle* h, TapeBlock& b, const char* who, const char* noun, Views& views, Layout layout,
                 DeviceBuf<double>* copy = nullptr, size_t copy_bytes = 0, bool keep = false) {
  Tape& t = h->tape;
  Views v{};
  const size_t bytes = keep ? b.bytes : layout(Carver{}, v);
  const size_t total = t.bytes - b.bytes + bytes + copy_bytes;
  const std::string what = std::string(who) + ": " + noun + " (" + std::to_string((keep ? 0 : bytes) + copy_bytes) + " bytes)";
  if (t.budget > 0 && total > (size_t)t.budget)
    return fail(h, PIC_ENOMEM, what + " would take the tape past budget_bytes (pic_tape_start)");
  DeviceBuf<void> mem;
  DeviceBuf<double> cmem;
  int rc = keep ? PIC_OK : regrow(h, mem, bytes, (what + " does not fit on the device").c_str());
  if (!rc && copy) rc = regrow(h, cmem, copy_bytes, (what + " does not fit on the device").c_str());
  if (rc) return rc;
  if (!keep) {
    if (b) HIPCHK(h, hipStreamSynchronize(h->stream));
    layout(Carver{static_cast<char*>(mem.get())}, v);
    b.mem = std::move(mem);
    b.bytes = bytes;
    views = v;
  }
  if (copy) *copy = std::move(cmem);
  t.bytes = total;
  return PIC_OK;
}

// a block of the tape goes again, and its bytes with it: for an entry that fails behind its tape_reserve
template <typename Attached>
void tape_release(Tape& t, Attached& a) {
  t.bytes -= a.block.bytes;
  a = Attached{};
}

// tape_reserve's sequence for a block of the handle that a call works on, outside any budget: `b` holds at least *cap bytes and
// grows to what `layout` needs (cap = null: the block is allocated as it is sized); the views are carved in any case.
template <typename Views, typename Layout>
int call_reserve(pic_handle* h, DeviceBuf<void>& b, size_t* cap, const char* who, const char* noun, Views& views, Layout layout) {
  Views v = views;
  const size_t bytes = layout(Carver{}, v);
  if (!cap || bytes > *cap) {
    if (cap) *cap = 0;
    const std::string what = std::string(who) + ": " + noun + " (" + std::to_string(bytes) + " bytes) does not fit on the device";
    if (int rc = regrow(h, b, bytes, what.c_str())) return rc;
    if (cap) *cap = bytes;
  }
  layout(Carver{static_cast<char*>(b.get())}, views);
  return PIC_OK;
}

// The tail of an entry that enqueued work: the first of `e` and the wait it asks for (wait: the call read something back to host
// memory) is the entry's PIC_EHIP
inline int hip_tail(pic_handle* h, hipError_t e, bool wait, const char* who) {
  const hipError_t e2 = wait ? hipStreamSynchronize(h->stream) : hipSuccess;
  if (e == hipSuccess) e = e2;
  return e == hipSuccess ? PIC_OK : fail(h, PIC_EHIP, std::string(who) + ": " + hipGetErrorString(e));
}

// the shape of a policy into the argument block of one of its three kernels (PolicyArgs, PolicyVjpArgs, PolicyJvpArgs; P: the
// doubles of one parameter vector)
template <typename Args>
void policy_shape(Args& a, const pic_policy& p, size_t P, double action_scale) {
  a.env_params = p.per_env ? (long long)P : 0;
  a.action_scale = action_scale;
  a.n_layers = p.n_layers;
  a.w0 = p.width[0]; a.w1 = p.width[1]; a.w2 = p.width[2]; a.w3 = p.width[3]; a.w4 = p.width[4];
  a.activation = p.activation; a.squash = p.squash;
}

// argument checks of the pic_tape_* entries
inline int check_mem_kind(pic_handle* h, int mem_kind, const char* who) {
  return mem_kind == PIC_HOST || mem_kind == PIC_DEVICE ? PIC_OK : fail(h, PIC_EINVAL, std::string(who) + ": bad mem_kind");
}
inline int check_tape_open(pic_handle* h, const char* who) {
  return h->tape.on ? PIC_OK : fail(h, PIC_ESTATE, std::string(who) + ": no tape is open (pic_tape_start)");
}
// the forward-mode entries that take no parameter direction stop at steps under an MLP policy (pic_tape_step_policy): their
// actions depend on the state through the network; pic_tape_tangent_policy (host_tangent_walk.h) is the entry for such a tape
inline int check_no_policy_steps(pic_handle* h, const char* who) {
  return h->tape.policy.calls.empty() ? PIC_OK
                             : fail(h, PIC_EINVAL, std::string(who) + ": the tape holds steps of pic_tape_step_policy (policy steps are "
                                                                      "not built in forward mode)");
}
// `what`, an argument that was given, needs the tape's a-bar rows
inline int check_tape_actuator(pic_handle* h, const void* given, const char* what, const char* who) {
  if (!given || h->tape.gact) return PIC_OK;
  return fail(h, PIC_ESTATE, std::string(who) + ": " + what + " needs an actuator set before pic_tape_start (pic_set_actuator)");
}
