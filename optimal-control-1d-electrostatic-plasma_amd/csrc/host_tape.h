// host_tape.h -- included by picstep.hip alone, inside its extern "C" block and ahead of advance, which calls tape_record_ext,
// tape_checkpoint and tape_kl_enqueue; behind host_moments.h (tape_moments_row, tape_moments_reverse)
#pragma once
// ---------------------------------------------------------------------------------------------
// Differentiable rollouts (include/picstep.h: pic_tape_*; kernels: pic_adjoint.h; hook: advance)
// ---------------------------------------------------------------------------------------------
// the forward sweeps' geometry and fixed point (sweep_args), the adjoint deposits' headroom and the Yoshida-4 coefficients
static AdjArgs adjoint_args(const pic_handle* h) {
  const SweepArgs s = sweep_args(h);
  AdjArgs a{};
  a.N = s.N; a.ld = s.ld; a.Ng = s.Ng; a.fg = s.fg; a.magic = s.magic;
  int b = 0;
  while (((int64_t)1 << b) < h->cfg.N) ++b;
  a.bitsN = b;
  a.L = s.L; a.dx = s.dx; a.dt = s.dt; a.scale = s.scale; a.N_over_L = s.N_over_L;
  for (int i = 0; i < 4; ++i) { a.c[i] = h->cs[i]; a.d[i] = h->ds[i]; }
  return a;
}

// e_t of n steps of `sc` into the tape (pic_adjoint.h: tape_ext_kernel)
static int tape_record_ext(pic_handle* h, const StepControl& sc, int n) {
  Tape& t = h->tape;
  TapeExtArgs a{};
  a.ext = sc.ctl.ext; a.act = sc.ctl.act; a.basis = sc.ctl.basis;
  a.out = t.ext + (size_t)t.steps * h->cfg.num_envs * h->cfg.Ng;
  a.ext_step = sc.ext_step; a.act_step = sc.act_step;
  a.Ng = h->cfg.Ng; a.M = sc.ctl.M; a.num_envs = h->cfg.num_envs;
  a.act_inline = sc.ctl.act && sc.inline_n > 0;
  hipLaunchKernelGGL(tape_ext_kernel, dim3(h->cfg.num_envs, n), dim3(ABLOCK), 0, h->stream, a, sc.inline_act);
  HIPCHK(h, hipGetLastError());
  return PIC_OK;
}

static int tape_checkpoint(pic_handle* h, int64_t c) {
  const size_t part = (size_t)h->cfg.num_envs * h->ld;
  double* dst = h->tape.ck + (size_t)c * 2 * part;
  HIPCHK(h, hipMemcpyAsync(dst, h->x, part * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(dst + part, h->v, part * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return PIC_OK;
}

int pic_tape_start(pic_handle* h, const pic_tape_config* c) {
  if (!h || !c) return fail(h, PIC_EINVAL, "pic_tape_start: null argument");
  if (h->tape.on) return fail(h, PIC_ESTATE, "pic_tape_start: a tape is open (pic_tape_stop first)");
  if (h->fmt != FMT_F64)
    return fail(h, PIC_EINVAL, "pic_tape_start: the tape needs float64 particles with float64 positions (float32 and fixed32 are "
                               "not differentiated)");
  if (h->acc_kind != PIC_ACC_FIX64)
    return fail(h, PIC_EINVAL, "pic_tape_start: the tape needs the 64-bit fixed-point accumulator (PIC_ACC_F64 sums depend on the "
                               "order of the adds, so a replay would not be bitwise)");
  if (h->cfg.interpol != PIC_CIC)
    return fail(h, PIC_EINVAL, "pic_tape_start: the tape needs CIC (the reference's TSC weights jump at cell edges: its cost is "
                               "not differentiable)");
  if (h->scheme != PIC_YOSHIDA4)
    return fail(h, PIC_EINVAL, "pic_tape_start: the tape differentiates the Yoshida-4 integrator only");
  if (c->max_steps < 1 || c->checkpoint_every < 0 || c->budget_bytes < 0)
    return fail(h, PIC_EINVAL, "pic_tape_start: need max_steps >= 1, checkpoint_every >= 0, budget_bytes >= 0");
  if (!h->has_state) return fail(h, PIC_ESTATE, "pic_tape_start: call pic_reset first");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, "pic_tape_start: a staged step is in progress");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int64_t every = c->checkpoint_every;
  const BlockDims d = block_dims(h);
  const auto tape_bytes = [&](int64_t ev) { TapeViews sized; return tape_parts(Carver{}, d, c->max_steps, ev, sized); };
  if (every == 0) {
    // about sqrt(max_steps) (checkpoints and one segment's replay weigh alike); when that exceeds budget_bytes, the interval
    // that needs the fewest bytes
    every = std::min<int64_t>(c->max_steps, std::max<int64_t>(1, (int64_t)std::ceil(std::sqrt((double)c->max_steps))));
    if (c->budget_bytes > 0 && tape_bytes(every) > (size_t)c->budget_bytes) {
      size_t best = tape_bytes(every);
      for (int64_t s = 1; s <= c->max_steps; ++s) {
        const size_t b = tape_bytes(s);
        if (b < best) { best = b; every = s; }
      }
    }
  }
  every = std::min<int64_t>(every, c->max_steps);
  Tape& t = h->tape;
  t = Tape{};
  t.budget = c->budget_bytes;
  int rc = tape_reserve<TapeViews>(h, t.block, "pic_tape_start", "the tape", t,
                                   [&](Carver cv, TapeViews& v) { return tape_parts(cv, d, c->max_steps, every, v); });
  if (rc) { t = Tape{}; return rc; }
  t.counters = t.cmax + h->cfg.num_envs;
  t.max_steps = c->max_steps; t.every = every; t.nck = c->max_steps / every + 1;
  hipError_t e = hipMemsetAsync(t.acc, 0, Carver::upto(t.acc, t.counters + 2), h->stream);    // acc, cmax, counters
  if (e != hipSuccess) { t = Tape{}; return hip_tail(h, e, false, "pic_tape_start"); }
  rc = tape_checkpoint(h, 0);
  if (rc) { t = Tape{}; return rc; }
  t.on = true;
  return PIC_OK;
}

int pic_tape_stop(pic_handle* h) {
  if (!h) return PIC_EINVAL;
  if (!h->tape.block) return PIC_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const hipError_t e = hipStreamSynchronize(h->stream);
  h->tape = Tape{};
  return hip_tail(h, e, false, "pic_tape_stop");
}

int pic_tape_stats(pic_handle* h, pic_tape_info* out) {
  if (!h || !out) return fail(h, PIC_EINVAL, "pic_tape_stats: null argument");
  std::memset(out, 0, sizeof(*out));
  const Tape& t = h->tape;
  if (!t.on) return PIC_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  unsigned long long cnt[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(cnt, t.counters, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  out->steps = t.steps;
  out->checkpoint_every = t.every;
  out->bytes = (int64_t)t.bytes;
  out->replay_mismatches = (int64_t)cnt[0];
  out->unit_retries = 0;              // the adjoint deposits' unit cannot overflow (pic_adjoint.h: adj_unit_exp)
  out->replay_bad_positions = (int64_t)cnt[1];
  out->launches = t.launches;
  return PIC_OK;
}

// step s of the open tape ran under the gain law
static bool tape_law_step(const pic_handle* h, int64_t s) {
  const Tape& t = h->tape;
  return s >= 0 && s < t.steps && !t.law.step.empty() && t.law.step[(size_t)s] >= 0;
}

// the gain law's record on an open tape (allocated by its first call) and one more gain of `gbytes`, within budget_bytes
static int tape_law_reserve(pic_handle* h, size_t gbytes) {
  Tape& t = h->tape;
  const bool first = !t.law.block;
  DeviceBuf<double> g;
  const int rc = tape_reserve<LawViews>(h, t.law.block, "pic_step_feedback_gain", "the law's record and this call's gain", t.law,
                                        [&](Carver c, LawViews& v) { return law_parts(c, block_dims(h), t.max_steps, v); }, &g, gbytes,
                                        !first);
  if (rc) return rc;
  t.law.gains.push_back(std::move(g));
  if (first) {
    t.law.step.assign((size_t)t.max_steps, -1);
    HIPCHK(h, hipMemsetAsync(t.law.modes, 0, Carver::upto(t.law.modes, t.law.cot), h->stream));
  }
  return PIC_OK;
}

// ---------------------------------------------------------------------------------------------
// The smoothed KL of every taped step (include/picstep.h: pic_tape_kl_*; hooks: advance, walk_reverse)
// ---------------------------------------------------------------------------------------------
int pic_tape_kl_start(pic_handle* h, const pic_phase_spec* s) {
  const char* who = "pic_tape_kl_start";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (int rc = check_tape_open(h, who)) return rc;
  if (t.kl.on) return fail(h, PIC_ESTATE, std::string(who) + ": the tape has a KL already");
  if (t.steps != 0) return fail(h, PIC_ESTATE, std::string(who) + ": the tape holds steps already (attach the KL before the first)");
  int rc = phase_check(h, s, PIC_HOST, who);
  if (rc) return rc;
  if (!s->feq) return fail(h, PIC_EINVAL, std::string(who) + ": needs spec->feq");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  rc = tape_reserve<KlViews>(h, t.kl.block, who, "the KL's memory", t.kl, [&](Carver c, KlViews& v) {
    return tape_kl_parts(c, block_dims(h), s->nx, s->nv, s->feq_per_env != 0, t.max_steps, v);
  });
  if (rc) return rc;
  const size_t fbytes = (s->feq_per_env ? (size_t)h->cfg.num_envs : 1) * s->nx * s->nv * sizeof(double);
  hipError_t e = hipMemcpyAsync(t.kl.feq, s->feq, fbytes, copy_kind(s->feq_mem_kind, hipMemcpyHostToDevice), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t.kl.acc, 0, Carver::upto(t.kl.acc, t.kl.g), h->stream);
  if (int rt = hip_tail(h, e, true, who)) {                          // (the caller's feq may go away behind this call)
    tape_release(t, t.kl);
    return rt;
  }
  t.kl.spec = *s;
  t.kl.spec.feq = t.kl.feq;
  t.kl.spec.feq_mem_kind = PIC_DEVICE;
  t.kl.flag.assign((size_t)t.max_steps, 0);
  t.kl.on = true;
  return PIC_OK;
}

// KL~ of the handle's particles into row t.steps of the trace (advance, behind the step that is about to be counted)
static int tape_kl_enqueue(pic_handle* h) {
  Tape& t = h->tape;
  PhaseArgs a;
  HIPCHK(h, phase_enqueue(h, &t.kl.spec, (const double*)h->x.get(), (const double*)h->v, t.kl.acc, t.kl.feq, nullptr, nullptr,
                          t.kl.trace + (size_t)t.steps * h->cfg.num_envs, nullptr, a));
  return PIC_OK;
}

// the KL's part of reverse step s (walk_reverse): lambda += k-bar_s dKL~/d(x', v') at the replayed state x', v' the step left
static int tape_kl_reverse(pic_handle* h, int64_t s, const double* x, const double* v, double* lx, double* lv) {
  Tape& t = h->tape;
  const int E = h->cfg.num_envs;
  const pic_phase_spec& sp = t.kl.spec;
  PhaseArgs a;
  HIPCHK(h, phase_enqueue(h, &sp, x, v, t.kl.acc, t.kl.feq, t.kl.cot + (size_t)s * E, nullptr, nullptr, t.kl.g, a));
  const double norm = phase_norm(h, &sp);
  const long long ntiles = (h->cfg.N + 1) / 2;
  const dim3 grid((unsigned)((ntiles + BLOCK - 1) / BLOCK), (unsigned)E);
  hipLaunchKernelGGL(phase_vjp_add_kernel, grid, dim3(BLOCK), 0, h->stream, x, v, (const double*)t.kl.g, a, norm * a.rdx,
                     norm * a.rdv, lx, lv);
  t.launches += 3;
  return PIC_OK;
}

int pic_tape_kl(pic_handle* h, int mem_kind, double* kl) {
  const char* who = "pic_tape_kl";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.kl.on) return fail(h, PIC_ESTATE, std::string(who) + ": no tape with a KL is open (pic_tape_kl_start)");
  if ((mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) || !kl) return fail(h, PIC_EINVAL, std::string(who) + ": bad mem_kind or null kl");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (t.steps == 0) return PIC_OK;
  HIPCHK(h, hipMemcpyAsync(kl, t.kl.trace, (size_t)t.steps * h->cfg.num_envs * sizeof(double), copy_kind(mem_kind, hipMemcpyDeviceToHost),
                           h->stream));
  if (mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_tape_kl_cot(pic_handle* h, const double* cot_kl, int mem_kind, int64_t first_step, int64_t nsteps) {
  const char* who = "pic_tape_kl_cot";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.kl.on) return fail(h, PIC_ESTATE, std::string(who) + ": no tape with a KL is open (pic_tape_kl_start)");
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (first_step < 0 || nsteps < 0 || first_step > t.steps || nsteps > t.steps - first_step)
    return fail(h, PIC_EINVAL, std::string(who) + ": rows outside the " + std::to_string(t.steps) + " steps taped so far");
  if (nsteps == 0) return PIC_OK;
  if (t.walk.on && first_step + nsteps - 1 > t.walk.next)
    return fail(h, PIC_ESTATE, std::string(who) + ": the walk in progress has reversed step " + std::to_string(first_step + nsteps - 1) +
                                   " already");
  if (cot_kl) {
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const size_t E = h->cfg.num_envs;
    HIPCHK(h, hipMemcpyAsync(t.kl.cot + (size_t)first_step * E, cot_kl, (size_t)nsteps * E * sizeof(double),
                             copy_kind(mem_kind, hipMemcpyHostToDevice), h->stream));
  }
  std::fill(t.kl.flag.begin() + first_step, t.kl.flag.begin() + first_step + nsteps, cot_kl ? 1 : 0);
  return PIC_OK;
}

// the fields of one replayed sub-stage: deposit in t.acc -> E (+ e_t) into `E_out`, the row cleared behind its read
static void tape_solve(pic_handle* h, const double* ext, double* E_out) {
  SolveIO io{};
  io.acc = h->tape.acc; io.acc_clear = h->tape.acc;
  io.out.ext = ext; io.out.E = E_out; io.out.num_envs = h->cfg.num_envs;
  // (not launch_solve: the replay's launches stay out of pic_profile's counters)
  hipLaunchKernelGGL(field_solve_kernel, dim3(h->cfg.num_envs), dim3(SBLOCK), h->solve_lds, h->stream, io, solve_args(h, 1));
  ++h->tape.launches;
}

// E-bar of the field step s started from (pic_adjoint.h: law_adjoint_kernel): the gain law's term if step s is a law step
// (e-bar_s must be complete), plus cot_m [env][2 mc] on its modes (either may be absent).  Returns where it went (t.law.E, or t.walk.E
// without a law block), or null: nothing to add.
static const double* tape_mode_cot(pic_handle* h, int64_t s, const double* cot_m, int mc) {
  Tape& t = h->tape;
  const bool lawstep = tape_law_step(h, s);
  if (!lawstep && !cot_m) return nullptr;
  double* Ebar = t.law.E ? t.law.E : t.walk.E;
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng, M = h->act_modes;
  const int mg = lawstep ? M : 0, R = std::max(mg, cot_m ? mc : 0);
  hipLaunchKernelGGL(law_adjoint_kernel, dim3(E), dim3(ABLOCK), (size_t)2 * (mg + R) * sizeof(double), h->stream,
                     lawstep ? (const double*)(t.gext + (size_t)s * E * Ng) : nullptr, (const double*)h->basis,
                     lawstep ? (const double*)t.law.gains[(size_t)t.law.step[(size_t)s]] : nullptr, cot_m, (const double*)h->tw, h->tw_rows,
                     Ebar, Ng, M, cot_m ? mc : 0);
  ++t.launches;
  return Ebar;
}

// the launch geometry of the reverse pass
struct WalkGeom {
  dim3 pgrid, mgrid;
  size_t acc_lds, mesh_lds;
};

static WalkGeom walk_geom(const pic_handle* h) {
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng;
  long long gx = (h->cfg.N + (long long)ABLOCK * 8 - 1) / ((long long)ABLOCK * 8);       // ~8 particles per lane
  gx = std::max<long long>(1, std::min<long long>(gx, std::max(1, 2048 / E)));
  return {dim3((unsigned)gx, E), dim3(E), (size_t)(Ng + 1) * sizeof(unsigned long long), (size_t)Ng * sizeof(double)};
}

// a walk from step T: lambda, e-bar, the counters and the launch count at zero; twiddles for M_o modes
static int walk_open(pic_handle* h, int mo) {
  Tape& t = h->tape;
  const size_t part = (size_t)h->cfg.num_envs * h->ld, mesh = (size_t)h->cfg.num_envs * h->cfg.Ng;
  t.walk.on = t.twalk.on = false;          // (a forward walk replays into the same segment buffer)
  t.policy.valid = false;
  const int mp = t.policy.block ? t.policy.shape.obs_modes : 0;      // a policy step's m-bar goes the way of a walk's mode cotangent
  if (mo > 0 || mp > 0) {
    const int rc = ensure_twiddle(h, std::max(mo, mp));
    if (rc) return rc;
    if (!t.law.E && !t.walk.E && alloc(t.walk.E, mesh * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, PIC_ENOMEM, "pic_tape_walk_begin: the walk's mode cotangent does not fit on the device");
    }
  }
  t.launches = 0;
  HIPCHK(h, hipMemsetAsync(t.counters, 0, 2 * sizeof(unsigned long long), h->stream));
  if (t.steps > 0) HIPCHK(h, hipMemsetAsync(t.gext, 0, (size_t)t.steps * mesh * sizeof(double), h->stream));
  HIPCHK(h, hipMemsetAsync(t.lam, 0, 2 * part * sizeof(double), h->stream));
  if (t.policy.block) HIPCHK(h, hipMemsetAsync(t.policy.gobs, 0, Carver::upto(t.policy.gobs, t.policy.cobs), h->stream));    // o-bar, u-bar, a-bar
  t.policy.first = true;
  t.policy.cot_obs = t.policy.cot_act = false;
  t.walk.on = true;
  t.walk.next = t.steps - 1;
  t.walk.mo = mo;
  return PIC_OK;
}

// restore the checkpoint of segment sgi into the replay states (never into the handle's x, v), replay it step by step and
// compare its end with the state the forward left there
static int walk_replay(pic_handle* h, int64_t sgi, const AdjArgs& a, const WalkGeom& g) {
  Tape& t = h->tape;
  const size_t part = (size_t)h->cfg.num_envs * h->ld, mesh = (size_t)h->cfg.num_envs * h->cfg.Ng;
  const int64_t nseg = (t.steps + t.every - 1) / t.every;
  const int64_t t0 = sgi * t.every, len = std::min<int64_t>(t.every, t.steps - t0);
  HIPCHK(h, hipMemcpyAsync(t.seg, t.ck + (size_t)sgi * 2 * part, 2 * part * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  for (int64_t i = 0; i < len; ++i) {
    const double* x = t.seg + (size_t)i * 2 * part;
    AdjStep st{x, x + part, t.F + (size_t)i * 3 * mesh, (long long)mesh};
    const double* e_t = t.ext + (size_t)(t0 + i) * mesh;
    double* xo = t.seg + (size_t)(i + 1) * 2 * part;
    hipLaunchKernelGGL(adjoint_replay_kernel<1>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, t.acc, nullptr, nullptr, a, t.counters + 1);
    tape_solve(h, e_t, t.F + (size_t)(i * 3 + 0) * mesh);
    hipLaunchKernelGGL(adjoint_replay_kernel<2>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, t.acc, nullptr, nullptr, a, t.counters + 1);
    tape_solve(h, e_t, t.F + (size_t)(i * 3 + 1) * mesh);
    hipLaunchKernelGGL(adjoint_replay_kernel<3>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, t.acc, nullptr, nullptr, a, t.counters + 1);
    tape_solve(h, e_t, t.F + (size_t)(i * 3 + 2) * mesh);
    hipLaunchKernelGGL(adjoint_replay_kernel<4>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, t.acc, xo, xo + part, a, t.counters + 1);
    tape_solve(h, nullptr, t.M + (size_t)i * mesh);
    t.launches += 4;
  }
  const double* end = t.seg + (size_t)len * 2 * part;
  const double* want_x = sgi + 1 < nseg ? t.ck + (size_t)(sgi + 1) * 2 * part : (const double*)h->x.get();
  const double* want_v = sgi + 1 < nseg ? want_x + part : (const double*)h->v;
  hipLaunchKernelGGL(tape_compare_kernel, g.pgrid, dim3(ABLOCK), 0, h->stream, end, end + part, want_x, want_v, h->cfg.N, h->ld, t.counters);
  ++t.launches;
  return PIC_OK;
}

// cotangents a reverse step injects, all on the device: on the modes of the field the step left (mc modes) and on the state it
// left (rows of cld elements); each may be null
struct WalkCot {
  const double* modes = nullptr;
  int mc = 0;
  const double* x = nullptr;
  const double* v = nullptr;
  long long cld = 0;
};

// The policy's part of a reverse pass: step s ran under an MLP policy and e-bar_s is complete.  a-bar_s = B^T
// e-bar_s (summed inside policy_vjp_kernel, in both of the gain law's orders: pic_policy.h) plus a backward's direct cotangent;
// the kernel gives u-bar_s, o-bar_s and adds the step's parameter terms to the per-environment sums; m-bar_s = o-bar_s plus a direct
// cotangent on the observation (a backward's row, or the walk's mode cotangent c.modes on the same field) replaces c.modes, so
// tape_mode_cot sends it through J^T as it sends a walk's.
static bool tape_policy_step(const pic_handle* h, int64_t s) {
  const Tape& t = h->tape;
  return s >= 0 && s < t.steps && !t.policy.step.empty() && t.policy.step[(size_t)s] >= 0;
}

static int tape_policy_reverse(pic_handle* h, int64_t s, WalkCot& c) {
  Tape& t = h->tape;
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng, M = h->act_modes, Mo = t.policy.shape.obs_modes;
  if (c.modes && c.mc != Mo)
    return fail(h, PIC_EINVAL, "pic_tape_walk: a mode cotangent on the field a policy step reads needs obs_modes = the policy's " +
                                   std::to_string(Mo) + " (pic_tape_walk_begin)");
  const size_t arow = (size_t)E * 2 * M, orow = (size_t)E * 2 * Mo;
  const Tape::Policy::Copy& pc = t.policy.calls[(size_t)t.policy.step[(size_t)s]];
  PolicyVjpArgs a{};
  a.obs = t.policy.obs + (size_t)s * orow;
  a.obs_scale = pc.scale;
  a.params = pc.params.get();
  a.pre = t.policy.pre + (size_t)s * arow;
  a.gext = t.gext + (size_t)s * E * Ng;
  a.basis = h->basis;
  a.Ng = Ng;
  a.cot_a2 = t.policy.cot_act ? t.policy.cact + (size_t)s * arow : nullptr;
  a.cot_obs = c.modes ? c.modes : (t.policy.cot_obs ? t.policy.cobs + (size_t)s * orow : nullptr);
  a.g_params = t.policy.gE;
  a.g_obs = t.policy.gobs + (size_t)s * orow;
  a.g_pre = t.policy.gpre + (size_t)s * arow;
  a.g_act = t.policy.gact + (size_t)s * arow;
  a.mbar = t.policy.mbar;
  a.P = (long long)t.policy.P;
  a.first = t.policy.first ? 1 : 0;
  a.Mo = Mo;
  policy_shape(a, t.policy.shape, t.policy.P, pc.action_scale);
  hipLaunchKernelGGL(policy_vjp_kernel, dim3(E), dim3(BLOCK), 0, h->stream, a);
  t.policy.first = false;
  ++t.launches;
  c.modes = t.policy.mbar;
  c.mc = Mo;
  return PIC_OK;
}

// reverse step t.walk.next (its energy cotangents in t.cot's row): first the replay of its segment if it is the segment's last step
static int walk_reverse(pic_handle* h, const WalkCot& given, const AdjArgs& a, const WalkGeom& g) {
  Tape& t = h->tape;
  const int E = h->cfg.num_envs;
  const size_t part = (size_t)E * h->ld, mesh = (size_t)E * h->cfg.Ng;
  const int64_t s = t.walk.next, sgi = s / t.every, t0 = sgi * t.every, i = s - t0;
  WalkCot c = given;
  if (tape_policy_step(h, s + 1)) {         // the policy of step s + 1 read the field step s left (nothing is enqueued if it fails)
    const int rc = tape_policy_reverse(h, s + 1, c);
    if (rc) return rc;
  }
  if (s + 1 == std::min<int64_t>(t0 + t.every, t.steps)) {
    const int rc = walk_replay(h, sgi, a, g);
    if (rc) return rc;
  }
  double* lx = t.lam;
  double* lv = t.lam + part;
  const double* x = t.seg + (size_t)i * 2 * part;
  const AdjStep st{x, x + part, t.F + (size_t)i * 3 * mesh, (long long)mesh};
  const double* cot = t.cot + (size_t)s * 3 * E;
  double* ge = t.gext + (size_t)s * mesh;
  if (t.kl.on && t.kl.flag[(size_t)s]) {       // lambda_x' += k-bar_s dKL~/dx', lambda_v' += k-bar_s dKL~/dv' 
    const double* xn = t.seg + (size_t)(i + 1) * 2 * part;
    const int rc = tape_kl_reverse(h, s, xn, xn + part, lx, lv);
    if (rc) return rc;
  }
  if (tape_moments_row(h, s)) {             // lambda' += the gather of m-bar_s at the replayed state step s left
    const double* xn = t.seg + (size_t)(i + 1) * 2 * part;
    tape_moments_reverse(h, s, xn, xn + part, lx, lv);
  }
  // the field step s left is read by the law of step s + 1 and by the caller's observation: E-bar joins its refresh adjoint
  const double* Ebar = tape_mode_cot(h, s + 1, c.modes, c.mc);
  hipLaunchKernelGGL(adjoint_mesh_kernel, g.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, nullptr, t.cmax, t.M + (size_t)i * mesh, cot, ge, t.nu, a, E,
                     Ebar);
  hipLaunchKernelGGL(adjoint_pass_kernel<3>, g.pgrid, dim3(ABLOCK), 0, h->stream, st, t.nu, cot, lx, lv, t.cmax, a, E, c.x, c.v, c.cld);
  hipLaunchKernelGGL(adjoint_deposit_kernel<3>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, lv, t.cmax, t.acc, a);
  hipLaunchKernelGGL(adjoint_mesh_kernel, g.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, t.acc, t.cmax, nullptr, nullptr, ge, t.nu, a, E, nullptr);
  hipLaunchKernelGGL(adjoint_pass_kernel<2>, g.pgrid, dim3(ABLOCK), 0, h->stream, st, t.nu, nullptr, lx, lv, t.cmax, a, E, nullptr, nullptr, 0ll);
  hipLaunchKernelGGL(adjoint_deposit_kernel<2>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, lv, t.cmax, t.acc, a);
  hipLaunchKernelGGL(adjoint_mesh_kernel, g.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, t.acc, t.cmax, nullptr, nullptr, ge, t.nu, a, E, nullptr);
  hipLaunchKernelGGL(adjoint_pass_kernel<1>, g.pgrid, dim3(ABLOCK), 0, h->stream, st, t.nu, nullptr, lx, lv, t.cmax, a, E, nullptr, nullptr, 0ll);
  hipLaunchKernelGGL(adjoint_deposit_kernel<1>, g.pgrid, dim3(ABLOCK), g.acc_lds, h->stream, st, lv, t.cmax, t.acc, a);
  hipLaunchKernelGGL(adjoint_mesh_kernel, g.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, t.acc, t.cmax, nullptr, nullptr, ge, t.nu, a, E, nullptr);
  hipLaunchKernelGGL(adjoint_pass_kernel<0>, g.pgrid, dim3(ABLOCK), 0, h->stream, st, t.nu, nullptr, lx, lv, t.cmax, a, E, nullptr, nullptr, 0ll);
  t.launches += 11;
  --t.walk.next;
  HIPCHK(h, hipGetLastError());
  return PIC_OK;
}

// after the last reverse step: the field at the tape start (read by a first law step and by the caller's observation c.modes)
// and the caller's cotangents on the starting state reach lambda_0 = (g_x0, g_v0)
static int walk_close(pic_handle* h, const WalkCot& given, const AdjArgs& a, const WalkGeom& g) {
  Tape& t = h->tape;
  const int E = h->cfg.num_envs;
  const size_t part = (size_t)E * h->ld;
  WalkCot c = given;
  if (tape_policy_step(h, 0)) {             // a first step under a policy read the field the tape started from
    const int rc = tape_policy_reverse(h, 0, c);
    if (rc) { t.walk.on = false; return rc; }
  }
  const double* Ebar = t.steps > 0 ? tape_mode_cot(h, 0, c.modes, c.mc) : nullptr;
  const bool field = Ebar != nullptr;
  if (field) {      // lambda_x0 += s W'(x_0) . K^T E-bar_0 at the tape-start positions
    hipLaunchKernelGGL(adjoint_mesh_kernel, g.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, nullptr, t.cmax, nullptr, nullptr, nullptr, t.nu, a, E,
                       Ebar);
    ++t.launches;
  }
  if (field || c.x || c.v) {
    hipLaunchKernelGGL(adjoint_start_kernel, g.pgrid, dim3(ABLOCK), 0, h->stream, (const double*)t.ck, field ? (const double*)t.nu : nullptr,
                       t.lam, a, t.lam + part, c.x, c.v, c.cld);
    ++t.launches;
  }
  if (tape_moments_row(h, -1)) tape_moments_reverse(h, -1, t.ck, t.ck + part, t.lam, t.lam + part);   // m-bar at the tape start
  t.walk.on = false;
  t.policy.valid = t.policy.block && !t.policy.first;
  HIPCHK(h, hipGetLastError());
  return PIC_OK;
}

// The end of a reverse pass or a tangent: lambda_0 to the caller's g_x0, g_v0 (each may be null).  Host memory: the call waits
// for the stream anyway, so a replay that left the forward's trajectory (particles written through pic_device_ptrs while
// taping) is PIC_ESTATE here, not only a count in pic_tape_stats: the gradient would be wrong
static int walk_finish(pic_handle* h, const std::string& w, int mem_kind, void* g_x0 = nullptr, void* g_v0 = nullptr) {
  int rc = g_x0 ? download(h, g_x0, h->tape.lam, mem_kind) : PIC_OK;
  if (!rc && g_v0) rc = download(h, g_v0, h->tape.lam + (size_t)h->cfg.num_envs * h->ld, mem_kind);
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  if (mem_kind != PIC_HOST) return PIC_OK;
  unsigned long long cnt = 0;
  HIPCHK(h, hipMemcpyAsync(&cnt, h->tape.counters, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (cnt)
    return fail(h, PIC_ESTATE, w + ": the replay differs from the taped forward in " + std::to_string((size_t)cnt) +
                                   " particle values (were the particles written while the tape was open?): the gradient is not valid");
  return PIC_OK;
}

// a-bar = B^T e-bar of steps [s0, s0 + n) to the caller's g_actions ([n][env][2M] in mem_kind's memory): straight into device
// memory, into host memory through the tape's own rows
static int tape_actions_out(pic_handle* h, int64_t s0, int64_t n, int mem_kind, double* g_actions) {
  Tape& t = h->tape;
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng, M = h->act_modes;
  const size_t arow = (size_t)E * 2 * M;
  double* out = device_output(g_actions, mem_kind, t.gact + (size_t)s0 * arow);
  hipLaunchKernelGGL(adjoint_actions_kernel, dim3(E, (unsigned)n), dim3(ABLOCK), 0, h->stream,
                     (const double*)(t.gext + (size_t)s0 * E * Ng), h->basis, out, Ng, M, E);
  ++t.launches;
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, device_result(h, g_actions, out, (size_t)n * arow * sizeof(double)));
  return PIC_OK;
}

// what pic_tape_backward_policy adds to a backward: direct cotangents on the policy steps' actions and observations (each may be
// null) and the per-step outputs (each may be null), all in the call's mem_kind
struct PolicyBackward {
  const double *cot_actions, *cot_obs;
  double *g_params, *g_pre, *g_obs, *g_actions;
};

// the accumulated parameter gradient to the caller's g_params: [env][P] with per_env, else the environments' sums added in
// ascending order
static int tape_policy_grad_out(pic_handle* h, int mem_kind, double* g_params) {
  Tape& t = h->tape;
  const size_t P = t.policy.P, E = (size_t)h->cfg.num_envs;
  const hipMemcpyKind outk = copy_kind(mem_kind, hipMemcpyDeviceToHost);
  if (t.policy.shape.per_env) {
    HIPCHK(h, hipMemcpyAsync(g_params, t.policy.gE, E * P * sizeof(double), outk, h->stream));
    return PIC_OK;
  }
  hipLaunchKernelGGL(policy_grad_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, (const double*)t.policy.gE, t.policy.g,
                     (long long)P, (int)E);
  ++t.launches;
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(g_params, t.policy.g, P * sizeof(double), outk, h->stream));
  return PIC_OK;
}

// the outputs of pic_tape_backward_policy behind the walk
static int tape_policy_out(pic_handle* h, int mem_kind, const PolicyBackward& pb) {
  Tape& t = h->tape;
  const size_t E = (size_t)h->cfg.num_envs, T = (size_t)t.steps, D = sizeof(double);
  const size_t arow = E * 2 * h->act_modes, orow = E * 2 * t.policy.shape.obs_modes;
  const hipMemcpyKind outk = copy_kind(mem_kind, hipMemcpyDeviceToHost);
  if (pb.g_params) {
    const int rc = tape_policy_grad_out(h, mem_kind, pb.g_params);
    if (rc) return rc;
  }
  if (T == 0) return PIC_OK;
  if (pb.g_pre) HIPCHK(h, hipMemcpyAsync(pb.g_pre, t.policy.gpre, T * arow * D, outk, h->stream));
  if (pb.g_obs) HIPCHK(h, hipMemcpyAsync(pb.g_obs, t.policy.gobs, T * orow * D, outk, h->stream));
  if (pb.g_actions) HIPCHK(h, hipMemcpyAsync(pb.g_actions, t.policy.gact, T * arow * D, outk, h->stream));
  return PIC_OK;
}

// the whole reverse pass in one call: a walk over every step with the whole trajectory's cotangents
static int tape_backward(pic_handle* h, const char* who, const double* cot_hist, const void* cot_x, const void* cot_v,
                         const double* cot_modes, int mem_kind, double* g_ext, double* g_actions, void* g_x0, void* g_v0,
                         double* modes_out, const PolicyBackward* pb = nullptr) {
  Tape& t = h->tape;
  const std::string w(who);
  if (int rc = check_tape_open(h, who)) return rc;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (int rc = check_tape_actuator(h, g_actions, "g_actions", who)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng;
  const int64_t T = t.steps;
  const size_t mesh = (size_t)E * Ng;
  const hipMemcpyKind outk = copy_kind(mem_kind, hipMemcpyDeviceToHost);
  const AdjArgs a = adjoint_args(h);
  const WalkGeom g = walk_geom(h);
  int rc = walk_open(h, 0);
  if (rc) return rc;
  if (T > 0) HIPCHK(h, device_fill(h, t.cot, cot_hist, (size_t)T * 3 * E * sizeof(double), mem_kind));
  if (cot_x) rc = upload(h, t.lam, cot_x, mem_kind);
  if (!rc && cot_v) rc = upload(h, t.lam + (size_t)E * h->ld, cot_v, mem_kind);
  if (rc) { t.walk.on = false; return rc; }
  if (pb && T > 0) {                  // the direct cotangents of the policy steps, read row by row by the walk
    const size_t arow = (size_t)E * 2 * h->act_modes, orow = (size_t)E * 2 * t.policy.shape.obs_modes;
    if (pb->cot_actions) {
      HIPCHK(h, device_fill(h, t.policy.cact, pb->cot_actions, (size_t)T * arow * sizeof(double), mem_kind));
      t.policy.cot_act = true;
    }
    if (pb->cot_obs) {
      HIPCHK(h, device_fill(h, t.policy.cobs, pb->cot_obs, (size_t)T * orow * sizeof(double), mem_kind));
      t.policy.cot_obs = true;
    }
  }
  // steps of the gain law: the action of step s + 1 depends on the field step s left, so the refresh adjoint of
  // step s also carries E-bar_{s+1} = J^T (G^T a-bar_{s+1} + m-bar_{s+1}); E-bar_0 reaches x_0 through the field at the start
  const bool law = !t.law.step.empty();
  const int M = h->act_modes;
  const size_t lrow = (size_t)E * 2 * M;
  if (law && T > 0) HIPCHK(h, device_fill(h, t.law.cot, cot_modes, (size_t)T * lrow * sizeof(double), mem_kind));
  // the law's m-bar of step s + 1 is a cotangent on the field step s left: the walk's mode cotangent of step s (law steps only)
  auto law_cot = [&](int64_t s) {
    WalkCot c;
    if (tape_law_step(h, s)) { c.modes = t.law.cot + (size_t)s * lrow; c.mc = M; }
    return c;
  };
  while (t.walk.next >= 0) {
    rc = walk_reverse(h, law_cot(t.walk.next + 1), a, g);
    if (rc) { t.walk.on = false; return rc; }
  }
  rc = walk_close(h, law_cot(0), a, g);
  if (rc) return rc;
  if (g_ext && T > 0) HIPCHK(h, hipMemcpyAsync(g_ext, t.gext, (size_t)T * mesh * sizeof(double), outk, h->stream));
  if (modes_out && T > 0) {
    if (law) HIPCHK(h, hipMemcpyAsync(modes_out, t.law.modes, (size_t)T * lrow * sizeof(double), outk, h->stream));
    else if (mem_kind == PIC_HOST) std::memset(modes_out, 0, (size_t)T * lrow * sizeof(double));
    else HIPCHK(h, hipMemsetAsync(modes_out, 0, (size_t)T * lrow * sizeof(double), h->stream));
  }
  if (g_actions && T > 0) rc = tape_actions_out(h, 0, T, mem_kind, g_actions);
  if (!rc && pb) rc = tape_policy_out(h, mem_kind, *pb);
  if (rc) return rc;
  return walk_finish(h, w, mem_kind, g_x0, g_v0);
}

int pic_tape_backward_policy(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, const double* cot_actions,
                             const double* cot_obs, int mem_kind, double* g_params, double* g_pre, double* g_obs, double* g_actions,
                             void* g_x0, void* g_v0) {
  const char* who = "pic_tape_backward_policy";
  if (!h) return PIC_EINVAL;
  if (int rc = check_tape_open(h, who)) return rc;
  if (!h->tape.policy.block) return fail(h, PIC_ESTATE, std::string(who) + ": the tape holds no steps of pic_tape_step_policy");
  const PolicyBackward pb{cot_actions, cot_obs, g_params, g_pre, g_obs, g_actions};
  return tape_backward(h, who, cot_hist, cot_x, cot_v, nullptr, mem_kind, nullptr, nullptr, g_x0, g_v0, nullptr, &pb);
}

int pic_tape_policy_grad(pic_handle* h, int mem_kind, double* g_params) {
  const char* who = "pic_tape_policy_grad";
  if (!h) return PIC_EINVAL;
  if (int rc = check_tape_open(h, who)) return rc;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (!g_params) return fail(h, PIC_EINVAL, std::string(who) + ": null g_params");
  Tape& t = h->tape;
  if (!t.policy.block) return fail(h, PIC_ESTATE, std::string(who) + ": the tape holds no steps of pic_tape_step_policy");
  if (!t.policy.valid)
    return fail(h, PIC_ESTATE, std::string(who) + ": no finished reverse pass over the steps taped so far (pic_tape_walk_end or a backward first)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int rc = tape_policy_grad_out(h, mem_kind, g_params);
  if (rc) return rc;
  if (mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}

int pic_tape_backward(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, int mem_kind, double* g_ext,
                      double* g_actions, void* g_x0, void* g_v0) {
  if (!h) return PIC_EINVAL;
  return tape_backward(h, "pic_tape_backward", cot_hist, cot_x, cot_v, nullptr, mem_kind, g_ext, g_actions, g_x0, g_v0, nullptr);
}

int pic_tape_backward_feedback(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, const double* cot_modes,
                               int mem_kind, double* g_ext, double* g_actions, void* g_x0, void* g_v0, double* modes_out) {
  if (!h) return PIC_EINVAL;
  if (int rc = check_tape_actuator(h, modes_out, "modes_out", "pic_tape_backward_feedback")) return rc;
  return tape_backward(h, "pic_tape_backward_feedback", cot_hist, cot_x, cot_v, cot_modes, mem_kind, g_ext, g_actions, g_x0, g_v0,
                       modes_out);
}

int pic_tape_walk_begin(pic_handle* h, int obs_modes, int mem_kind) {
  if (!h) return PIC_EINVAL;
  if (int rc = check_tape_open(h, "pic_tape_walk_begin")) return rc;
  if (obs_modes < 1 || obs_modes >= h->cfg.Ng) return fail(h, PIC_EINVAL, "pic_tape_walk_begin: need 1 <= obs_modes < N_mesh");
  if (int rc = check_mem_kind(h, mem_kind, "pic_tape_walk_begin")) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return walk_open(h, obs_modes);
}

// the cotangents a walk call injects (mem_kind's pointers; rows of N elements); host ones are staged on the device through
// wstage: [2][env][N] particles, then [env][2 M_o] modes
static int walk_cot(pic_handle* h, const void* cot_x, const void* cot_v, const double* cot_modes, bool host, WalkCot* c) {
  Tape& t = h->tape;
  const size_t E = h->cfg.num_envs, N = h->cfg.N;
  c->x = static_cast<const double*>(cot_x);
  c->v = static_cast<const double*>(cot_v);
  c->modes = cot_modes;
  c->mc = t.walk.mo;
  c->cld = (long long)N;
  if (!host || !(cot_x || cot_v || cot_modes)) return PIC_OK;
  const size_t bytes = (2 * E * N + E * 2 * t.walk.mo) * sizeof(double);
  if (bytes > t.walk.stage_bytes) {
    t.walk.stage_bytes = 0;
    const int rc = regrow(h, t.walk.stage, bytes, "pic_tape_walk: the staging of host cotangents does not fit on the device");
    if (rc) return rc;
    t.walk.stage_bytes = bytes;
  }
  double* st = t.walk.stage;
  HIPCHK(h, device_input(h, c->x, PIC_HOST, E * N * sizeof(double), st, &c->x));
  HIPCHK(h, device_input(h, c->v, PIC_HOST, E * N * sizeof(double), st + E * N, &c->v));
  HIPCHK(h, device_input(h, c->modes, PIC_HOST, E * 2 * t.walk.mo * sizeof(double), st + 2 * E * N, &c->modes));
  return PIC_OK;
}

int pic_tape_walk_step(pic_handle* h, const double* cot_energies, const void* cot_x, const void* cot_v, const double* cot_modes,
                       int mem_kind, double* g_ext, double* g_actions, int64_t* step) {
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.walk.on) return fail(h, PIC_ESTATE, "pic_tape_walk_step: no walk in progress (pic_tape_walk_begin)");
  if (t.walk.next < 0) return fail(h, PIC_ESTATE, "pic_tape_walk_step: every step has been walked (pic_tape_walk_end)");
  if (int rc = check_mem_kind(h, mem_kind, "pic_tape_walk_step")) return rc;
  if (int rc = check_tape_actuator(h, g_actions, "g_actions", "pic_tape_walk_step")) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs;
  const int64_t s = t.walk.next;
  const size_t mesh = (size_t)E * h->cfg.Ng;
  const bool host = mem_kind == PIC_HOST;
  double* cot = t.cot + (size_t)s * 3 * E;
  HIPCHK(h, device_fill(h, cot, cot_energies, 3 * E * sizeof(double), mem_kind));
  WalkCot c;
  int rc = walk_cot(h, cot_x, cot_v, cot_modes, host, &c);
  if (rc) return rc;
  rc = walk_reverse(h, c, adjoint_args(h), walk_geom(h));
  if (rc) { t.walk.on = false; return rc; }
  if (g_ext) HIPCHK(h, hipMemcpyAsync(g_ext, t.gext + (size_t)s * mesh, mesh * sizeof(double), copy_kind(mem_kind, hipMemcpyDeviceToHost), h->stream));
  if (g_actions) rc = tape_actions_out(h, s, 1, mem_kind, g_actions);      // a-bar_s = B^T e-bar_s of this step alone
  if (rc) return rc;
  if (host && (g_ext || g_actions)) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (step) *step = s;
  return PIC_OK;
}

int pic_tape_walk_end(pic_handle* h, const void* cot_x0, const void* cot_v0, const double* cot_modes0, int mem_kind, void* g_x0,
                      void* g_v0) {
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.walk.on) return fail(h, PIC_ESTATE, "pic_tape_walk_end: no walk in progress (pic_tape_walk_begin)");
  if (t.walk.next >= 0)
    return fail(h, PIC_ESTATE, "pic_tape_walk_end: " + std::to_string(t.walk.next + 1) + " steps are not walked yet (pic_tape_walk_step)");
  if (int rc = check_mem_kind(h, mem_kind, "pic_tape_walk_end")) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  WalkCot c;
  int rc = walk_cot(h, cot_x0, cot_v0, cot_modes0, mem_kind == PIC_HOST, &c);
  if (rc) { t.walk.on = false; return rc; }
  rc = walk_close(h, c, adjoint_args(h), walk_geom(h));
  return rc ? rc : walk_finish(h, "pic_tape_walk_end", mem_kind, g_x0, g_v0);
}
