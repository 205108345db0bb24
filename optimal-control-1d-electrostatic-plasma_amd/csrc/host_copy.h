// host_copy.h -- the host side of pic_copy_envs (kernels: pic_copy.h; the host map's check: host_copy_map.h).
// Included by picstep.hip inside its extern "C" block.

// what two handles must share for the state of one to be a state of the other: empty, or the name of the first field that differs
static std::string copy_mismatch(const pic_handle* d, const pic_handle* s) {
  if (d->cfg.N != s->cfg.N) return "N";
  if (d->cfg.Ng != s->cfg.Ng) return "Ng";
  if (d->cfg.L != s->cfg.L) return "L";
  if (d->cfg.n0 != s->cfg.n0) return "n0";
  if (d->cfg.dt != s->cfg.dt) return "dt";
  if (d->cfg.particle_dtype != s->cfg.particle_dtype) return "particle_dtype";
  if (d->cfg.position_dtype != s->cfg.position_dtype) return "position_dtype";
  if (d->cfg.interpol != s->cfg.interpol) return "interpol";
  if (d->acc_kind != s->acc_kind) return "accum_dtype";
  if (d->scheme != s->scheme) return "integrator";
  if (d->cfg.device_id != s->cfg.device_id) return "device_id";
  return "";
}

int pic_copy_envs(pic_handle* dst, pic_handle* src, const int32_t* map, int mem_kind) {
  if (!dst || !src) return fail(dst, PIC_EINVAL, "pic_copy_envs: null handle");
  pic_handle* h = dst;
  const bool same = src == dst;
  if (mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) return fail(h, PIC_EINVAL, "pic_copy_envs: mem_kind must be PIC_HOST or PIC_DEVICE");
  if (!same) {
    const std::string what = copy_mismatch(dst, src);
    if (!what.empty())
      return fail(h, PIC_EINVAL, "pic_copy_envs: the two handles differ in " + what + " (a copy needs the same N, Ng, L, n0, dt, "
                                 "particle and position dtype, interpol, accum_dtype, integrator and device)");
  }
  if (!src->has_state) return fail(h, PIC_ESTATE, "pic_copy_envs: the source holds no state (call pic_reset on it first)");
  if (src->sched.mid_stage || dst->sched.mid_stage)
    return fail(h, PIC_ESTATE, "pic_copy_envs: a staged step is in progress (finish its pic_step_stage calls)");
  if (dst->tape.on || dst->tape.walk.on)
    return fail(h, PIC_ESTATE, "pic_copy_envs: refused while a tape is open on the destination (pic_tape_stop first)");
  const int E = dst->cfg.num_envs, Es = src->cfg.num_envs, Ng = h->cfg.Ng;
  const bool host_map = mem_kind == PIC_HOST || !map;
  // (an entry the kernels refuse keeps its environment: there must be one to keep)
  if (!host_map && !dst->has_state)
    return fail(h, PIC_ESTATE, "pic_copy_envs: a device map needs a destination that holds state (an entry the kernels refuse "
                               "keeps its environment); reset it, or copy with a host map first");
  if (host_map) {
    const std::string bad = check_copy_map(map, E, Es, same);
    if (!bad.empty()) return fail(h, PIC_EINVAL, "pic_copy_envs: " + bad);
  }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (!h->copy_rejected) HIPCHK(h, alloc_zeroed(h->copy_rejected, sizeof(unsigned long long), h->stream));
  const int* dmap = map;
  if (map && mem_kind == PIC_HOST) {
    if (!h->copy_map) HIPCHK(h, alloc(h->copy_map, (size_t)E * sizeof(int)));
    HIPCHK(h, hipMemcpyAsync(h->copy_map, map, (size_t)E * sizeof(int), hipMemcpyHostToDevice, h->stream));
    dmap = h->copy_map;
  }
  const bool two_streams = !same && src->stream != dst->stream;
  if (two_streams) {                   // the copy reads what the source's stream has written ...
    for (EventOwner& ev : h->copy_ev)
      if (!ev) {
        hipEvent_t e = nullptr;
        HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.reset(e);
      }
    HIPCHK(h, hipEventRecord(h->copy_ev[0], src->stream));
    HIPCHK(h, hipStreamWaitEvent(dst->stream, h->copy_ev[0], 0));
  }

  // Which caches travel.  A cache is copied where both handles lay it out alike; the destination must also hold one already
  // unless the host has checked the map (an entry a device map gets wrong keeps its environment, and that environment's part of
  // a cache it never had would be zeros).  Everything else is dropped as pic_invalidate drops it: integer sums, the same bits.
  const bool fills_all = same || host_map;
  bool ring = src->sched.q_slot >= 0 && dst->S == src->S && dst->resident == src->resident && (dst->sched.q_slot >= 0 || fills_all);
  bool q1 = src->resident && dst->resident && src->res_q1_valid && dst->res_R == src->res_R && dst->res_lean == src->res_lean &&
            (dst->res_q1_valid || fills_all);
  bool carry = q1 && src->res_carry_valid && dst->res_carry && src->res_carry &&
               dst->res_carry_bytes / E == src->res_carry_bytes / Es && (dst->res_carry_valid || fills_all);
  if (!same) {
    if (ring && dst->sched.q_slot < 0) dst->sched.q_slot = ring_take_clean(dst);
    if (!ring) { dst->sched.ring.retire(dst->sched.q_slot); dst->sched.q_slot = -1; }
    dst->res_q1_valid = q1;
    dst->res_carry_valid = carry;
  }

  CopySmallArgs sm{};
  sm.map = dmap; sm.E_src = Es; sm.same = same ? 1 : 0; sm.rejected = h->copy_rejected;
  int k = 0;
  auto words = [](const void* p) { return static_cast<const unsigned long long*>(p); };
  auto seg = [&](const void* s, void* d, long long s_env, long long d_env, int n, int nsub = 1, long long s_sub = 0, long long d_sub = 0) {
    sm.s[k++] = CopySeg{words(s), static_cast<unsigned long long*>(d), s_env, d_env, s_sub, d_sub, n, nsub};
  };
  seg(src->n, dst->n, Ng, Ng, Ng);
  seg(src->E_mesh, dst->E_mesh, Ng, Ng, Ng);
  seg(src->phi, dst->phi, Ng, Ng, Ng);
  seg(src->KE, dst->KE, 1, 1, 1);
  seg(src->PE, dst->PE, 1, 1, 1);
  seg(src->PEr, dst->PEr, 1, 1, 1);
  if (ring) seg(ring_row(src, src->sched.q_slot), ring_row(dst, dst->sched.q_slot), Ng, Ng, Ng, dst->S, (long long)Es * Ng, (long long)E * Ng);
  if (q1) {
    const int w = dst->res_R * (Ng + 2);
    seg(src->res_q1, dst->res_q1, w, w, w);
  }

  CopyRowsArgs ra{};
  ra.map = dmap; ra.E_src = Es; ra.same = sm.same;
  const long long row = (long long)h->ld * (long long)h->esz;
  ra.a[0] = CopyRowSet{static_cast<const char*>(src->x.get()), static_cast<char*>(dst->x.get()), row, row, row / 16};
  ra.a[1] = CopyRowSet{static_cast<const char*>(src->v), static_cast<char*>(dst->v), row, row, row / 16};
  int narr = 2;
  long long nvec = row / 16;
  if (carry) {
    const long long cb = (long long)(dst->res_carry_bytes / E);
    ra.a[2] = CopyRowSet{static_cast<const char*>(src->res_carry.get()), static_cast<char*>(dst->res_carry.get()), cb, cb, cb / 16};
    narr = 3;
    if (cb / 16 > nvec) nvec = cb / 16;
  }
  const long long round = (long long)kCopyBlock * kCopyUnroll;
  const unsigned chunks = (unsigned)std::min<long long>((nvec + round - 1) / round, 65535);
  // (environments first: the workgroups of one source chunk are neighbours in launch order, pic_copy.h)
  prof_begin(h, 5);
  hipLaunchKernelGGL(copy_rows_kernel, dim3(E, chunks, narr), dim3(kCopyBlock), 0, h->stream, ra);
  hipLaunchKernelGGL(copy_env_small_kernel, dim3(E), dim3(kCopyBlock), 0, h->stream, sm);
  prof_end(h);
  const hipError_t launched = launch_status(h);
  if (launched != hipSuccess) drop_cached_deposits(dst);      // no cache may outlive a copy that did not go out whole
  HIPCHK(h, launched);
  dst->has_state = true;
  if (two_streams) {                   // ... and a later step of the source must not overtake that read
    HIPCHK(h, hipEventRecord(h->copy_ev[1], dst->stream));
    HIPCHK(h, hipStreamWaitEvent(src->stream, h->copy_ev[1], 0));
  }
  return PIC_OK;
}

int pic_copy_envs_rejected(pic_handle* h, int64_t* count) {
  if (!h || !count) return PIC_EINVAL;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  unsigned long long c = 0;
  if (h->copy_rejected) HIPCHK(h, hipMemcpyAsync(&c, h->copy_rejected, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *count = (int64_t)c;
  return PIC_OK;
}
