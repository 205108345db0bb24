// host_tangent.h -- included by picstep.hip alone, inside its extern "C" block, behind host_tape.h (the replay is the walk's)
#pragma once
// ---------------------------------------------------------------------------------------------
// Forward mode of the tape (include/picstep.h: pic_tape_tangent[_kl]; kernels: pic_tangent.h), of its per-step
// smoothed KL (kernels: pic_phase.h) and of its per-step moments (kernels: pic_moments.h)
// ---------------------------------------------------------------------------------------------
// the tangent block for K directions, within budget_bytes (grown for more; on failure the tape keeps what it had)
static int tangent_reserve(pic_handle* h, int K, const char* who) {
  Tape& t = h->tape;
  if (t.tan.k >= K) return PIC_OK;
  const int rc = tape_reserve(h, t.tan.block, who, "the tangent's working memory", t.tan.views,
                              [&](Carver c, TanArgs& v) { return tangent_parts(c, block_dims(h), K, v); });
  if (!rc) t.tan.k = K;
  return rc;
}

// the tangent block's views for K live directions, into the kernels' argument block
static TanArgs tangent_args(const pic_handle* h, int K) {
  const size_t part = (size_t)h->cfg.num_envs * h->ld;
  TanArgs ta = h->tape.tan.views;
  ta.dstride = (long long)(2 * part); ta.vofs = (long long)part;
  ta.K = K; ta.num_envs = h->cfg.num_envs;
  return ta;
}

// (dx_0, dv_0) of ta.K directions from the caller's [K][env][N] (each may be null: 0) into the state rows (padded to ld)
static int tangent_state_in(pic_handle* h, const TanArgs& ta, const void* d_x0, const void* d_v0, int mem_kind) {
  const size_t part = (size_t)h->cfg.num_envs * h->ld, EN = (size_t)h->cfg.num_envs * h->cfg.N;
  const void* ins[2] = {d_x0, d_v0};
  for (int d = 0; d < ta.K; ++d)
    for (int k = 0; k < 2; ++k) {
      double* dst = ta.st + (size_t)d * 2 * part + (size_t)k * part;
      if (!ins[k]) HIPCHK(h, hipMemsetAsync(dst, 0, part * sizeof(double), h->stream));
      else if (int rc = upload(h, dst, static_cast<const double*>(ins[k]) + (size_t)d * EN, mem_kind)) return rc;
    }
  return PIC_OK;
}

// (dx, dv) of every direction out of the state rows to the caller's [K][env][N] (each may be null)
static int tangent_state_out(pic_handle* h, const TanArgs& ta, int mem_kind, void* d_x, void* d_v) {
  const size_t part = (size_t)h->cfg.num_envs * h->ld, EN = (size_t)h->cfg.num_envs * h->cfg.N;
  void* outs[2] = {d_x, d_v};
  for (int d = 0; d < ta.K; ++d)
    for (int k = 0; k < 2; ++k)
      if (outs[k])
        if (int rc = download(h, static_cast<double*>(outs[k]) + (size_t)d * EN, ta.st + (size_t)d * 2 * part + (size_t)k * part, mem_kind)) return rc;
  return PIC_OK;
}

// the block behind the KL's tangent (kMaxTangents directions), within budget_bytes (allocated once per tape)
static int tangent_kl_reserve(pic_handle* h, const char* who) {
  Tape& t = h->tape;
  if (t.tkl.block) return PIC_OK;
  BlockDims d = block_dims(h);
  d.chunks = (size_t)phase_jvp_chunks(h);
  const int rc = tape_reserve<TanKlViews>(h, t.tkl.block, who, "the working memory of the KL's tangent", t.tkl,
                                          [&](Carver c, TanKlViews& v) { return tangent_kl_parts(c, d, kMaxTangents, v); });
  if (rc) return rc;
  const hipError_t e = phase_fill_ones(h, t.tkl.ones, (size_t)h->cfg.num_envs);
  if (e != hipSuccess) tape_release(t, t.tkl);
  return hip_tail(h, e, false, who);
}

// the KL's part of forward step s (kKlTangentLaunches kernels): the deposit and finish of the replayed state x, v the step left,
// with unit cotangents, then d_kl[d][s][env] = <dKL~/d(x', v'), (dq_4, dp_3)> on the tangent state after pass 3
constexpr int kKlTangentLaunches = 4;
static int tangent_kl_step(pic_handle* h, const TanArgs& ta, const double* x, const double* v, double* out, long long out_dstride) {
  Tape& t = h->tape;
  PhaseArgs a;
  HIPCHK(h, phase_enqueue(h, &t.kl.spec, x, v, t.kl.acc, t.kl.feq, t.tkl.ones, nullptr, nullptr, t.kl.g, a));
  PhaseJvpArgs j{};
  j.dx = ta.st; j.dv = ta.st + ta.vofs; j.dstride = ta.dstride; j.erow = h->ld; j.part = t.tkl.part;
  HIPCHK(h, phase_jvp_enqueue(h, &t.kl.spec, a, x, v, t.kl.g, j, ta.K, out, out_dstride));
  t.launches += kKlTangentLaunches;
  return PIC_OK;
}

// the working memory behind the moments' tangents (kMaxTangents directions), within budget_bytes (allocated once per tape)
static int tangent_moments_reserve(pic_handle* h, const char* who) {
  Tape& t = h->tape;
  if (t.tmom.block) return PIC_OK;
  return tape_reserve(h, t.tmom.block, who, "the working memory of the moments' tangent", t.tmom.views,
                      [&](Carver c, MomJvpArgs& v) { return moments_jvp_parts(c, block_dims(h), kMaxTangents, v); });
}

// the moments' part of forward step s (kMomentsJvpLaunches kernels): d_moments[d][s] = the tangent of the moments of the replayed
// state x, v the step left, along the tangent state after pass 3, (dq_4, dp_3) = (dx', dv')
static int tangent_moments_step(pic_handle* h, const TanArgs& ta, const double* x, const double* v, double* out, long long out_dstride) {
  Tape& t = h->tape;
  MomJvpArgs j = t.tmom.views;
  j.dx = ta.st; j.dv = ta.st + ta.vofs; j.dstride = ta.dstride; j.erow = h->ld;
  HIPCHK(h, moments_jvp_enqueue(h, x, v, j, ta.K, out, out_dstride));
  t.launches += kMomentsJvpLaunches;
  return PIC_OK;
}

extern "C++" {
// the kernels of a sub-stage for the direction count at hand (1, up to 4, up to 8: the per-direction values live in registers)
template <int S>
static void tangent_deposit(pic_handle* h, const AdjStep& st, const TanArgs& ta, const AdjArgs& a, dim3 grid, size_t lds, int kd) {
  if (kd == 1) hipLaunchKernelGGL((tangent_deposit_kernel<S, 1>), grid, dim3(ABLOCK), lds, h->stream, st, ta, a, kd);
  else if (kd <= 4) hipLaunchKernelGGL((tangent_deposit_kernel<S, 4>), grid, dim3(ABLOCK), lds, h->stream, st, ta, a, kd);
  else hipLaunchKernelGGL((tangent_deposit_kernel<S, 8>), grid, dim3(ABLOCK), lds, h->stream, st, ta, a, kd);
}

template <int S>
static void tangent_pass(pic_handle* h, const AdjStep& st, const TanArgs& ta, const AdjArgs& a, dim3 grid) {
  if (ta.K == 1) hipLaunchKernelGGL((tangent_pass_kernel<S, 1>), grid, dim3(ABLOCK), 0, h->stream, st, ta, a);
  else if (ta.K <= 4) hipLaunchKernelGGL((tangent_pass_kernel<S, 4>), grid, dim3(ABLOCK), 0, h->stream, st, ta, a);
  else hipLaunchKernelGGL((tangent_pass_kernel<S, 8>), grid, dim3(ABLOCK), 0, h->stream, st, ta, a);
}
}  // extern "C++"

// the launch geometry of a forward-mode step: a deposit workgroup holds kd directions' meshes in 64 KB of LDS; groups of them run
// side by side (grid z); one mesh workgroup per (environment, direction)
struct TanGeom {
  int kd;
  dim3 dgrid, mgrid;
  size_t dlds;
};

static TanGeom tangent_geom(const pic_handle* h, const WalkGeom& g, int K) {
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng;
  const int kd = std::min<int>(K, (int)std::max<size_t>(1, 65536 / ((size_t)(Ng + 1) * sizeof(unsigned long long))));
  return {kd, dim3(g.pgrid.x, E, (K + kd - 1) / kd), dim3(E, K), (size_t)kd * (Ng + 1) * sizeof(unsigned long long)};
}

// Forward-mode step i of the replayed segment (pic_tape_tangent, the tangent walk and pic_tape_tangent_feedback all advance
// through here): deposit -> mesh -> pass for the sub-stages 1..3, then the deposit and mesh of the state the step left.  m: the
// step's injection and outputs (its M is set here).  dkl / dmom: direction 0's row of this step, or null.
static int tangent_step(pic_handle* h, const TanArgs& ta, const AdjArgs& a, const WalkGeom& g, const TanGeom& tg, int64_t i, TanMeshIO m,
                        double* dkl, long long kl_dstride, double* dmom, long long mom_dstride) {
  Tape& t = h->tape;
  const size_t part = (size_t)h->cfg.num_envs * h->ld, mesh = (size_t)h->cfg.num_envs * h->cfg.Ng;
  const double* x = t.seg + (size_t)i * 2 * part;
  const AdjStep st{x, x + part, t.F + (size_t)i * 3 * mesh, (long long)mesh};
  m.M = t.M + (size_t)i * mesh;
  tangent_deposit<1>(h, st, ta, a, tg.dgrid, tg.dlds, tg.kd);
  hipLaunchKernelGGL(tangent_mesh_kernel<1>, tg.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, ta, m, a);
  tangent_pass<1>(h, st, ta, a, g.pgrid);
  tangent_deposit<2>(h, st, ta, a, tg.dgrid, tg.dlds, tg.kd);
  hipLaunchKernelGGL(tangent_mesh_kernel<2>, tg.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, ta, m, a);
  tangent_pass<2>(h, st, ta, a, g.pgrid);
  tangent_deposit<3>(h, st, ta, a, tg.dgrid, tg.dlds, tg.kd);
  hipLaunchKernelGGL(tangent_mesh_kernel<3>, tg.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, ta, m, a);
  tangent_pass<3>(h, st, ta, a, g.pgrid);
  if (dkl) {                        // the state is (dq_4, dp_3) = (dx', dv'): the tangent of the KL~ of the state the step left
    const double* xn = t.seg + (size_t)(i + 1) * 2 * part;
    if (int rc = tangent_kl_step(h, ta, xn, xn + part, dkl, kl_dstride)) return rc;
  }
  if (dmom) {                       // the same tangent state against the same replayed state: the moments' tangents (7l)
    const double* xn = t.seg + (size_t)(i + 1) * 2 * part;
    if (int rc = tangent_moments_step(h, ta, xn, xn + part, dmom, mom_dstride)) return rc;
  }
  tangent_deposit<4>(h, st, ta, a, tg.dgrid, tg.dlds, tg.kd);
  hipLaunchKernelGGL(tangent_mesh_kernel<4>, tg.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, ta, m, a);
  t.launches += 11;
  return PIC_OK;
}

// pic_tape_tangent (d_kl = null: the KL, if any, is ignored), pic_tape_tangent_kl and pic_tape_tangent_moments (d_moments = null:
// no kernel, byte or launch of the moments')
static int tape_tangent(pic_handle* h, const char* who, int K, const double* d_ext, const double* d_actions, const void* d_x0,
                        const void* d_v0, int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh, double* d_kl,
                        double* d_moments = nullptr) {
  Tape& t = h->tape;
  const std::string w(who);
  if (int rc = check_tape_open(h, w.c_str())) return rc;
  if (int rc = check_no_policy_steps(h, w.c_str())) return rc;
  if (d_kl && !t.kl.on) return fail(h, PIC_ESTATE, w + ": d_kl needs a KL on the tape (pic_tape_kl_start before the first step)");
  if (K < 1 || K > kMaxTangents) return fail(h, PIC_EINVAL, w + ": need 1 <= K <= " + std::to_string(kMaxTangents));
  if (d_ext && d_actions) return fail(h, PIC_EINVAL, w + ": d_ext and d_actions are both given (at most one)");
  if (int rc = check_mem_kind(h, mem_kind, w.c_str())) return rc;
  const int64_t T = t.steps;
  for (int64_t s = 0; s < T; ++s)
    if (tape_law_step(h, s))
      return fail(h, PIC_ESTATE, w + ": the tape holds steps of pic_step_feedback_gain, and forward mode through the gain law is "
                                     "not built (pic_tape_backward_feedback differentiates it in reverse)");
  if (int rc = check_tape_actuator(h, d_actions, "d_actions", w.c_str())) return rc;
  if (d_moments)
    if (int rc = moments_jvp_check(h, w)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng, Mact = h->act_modes;
  const bool host = mem_kind == PIC_HOST;
  const size_t N = h->cfg.N, mesh = (size_t)E * Ng, row = N * sizeof(double);
  t.walk.on = t.twalk.on = false;           // (a walk's replayed segment is about to be overwritten)
  t.launches = 0;
  HIPCHK(h, hipMemsetAsync(t.counters, 0, 2 * sizeof(unsigned long long), h->stream));
  if (T == 0) {                       // no step: the tangent of the final particles is the initial one (NULL: 0)
    const size_t n = (size_t)K * E * row;
    void* outs[2] = {d_x, d_v};
    const void* ins[2] = {d_x0, d_v0};
    for (int k = 0; k < 2; ++k) {
      if (!outs[k]) continue;
      if (!host) HIPCHK(h, device_fill(h, static_cast<double*>(outs[k]), static_cast<const double*>(ins[k]), n, mem_kind));
      else if (ins[k]) std::memcpy(outs[k], ins[k], n);
      else std::memset(outs[k], 0, n);
    }
    if (host) HIPCHK(h, hipStreamSynchronize(h->stream));
    return PIC_OK;
  }
  int rc = tangent_reserve(h, K, who);
  if (!rc && d_kl) rc = tangent_kl_reserve(h, who);
  if (!rc && d_moments) rc = tangent_moments_reserve(h, who);
  if (rc) return rc;
  if (d_moments)                       // (a failed call may leave sums or max words)
    HIPCHK(h, hipMemsetAsync(t.tmom.views.acc, 0, Carver::upto(t.tmom.views.acc, t.tmom.views.umax + 3 * (size_t)kMaxTangents * E), h->stream));
  const TanArgs ta = tangent_args(h, K);
  HIPCHK(h, hipMemsetAsync(ta.acc, 0, Carver::upto(ta.acc, ta.umax + 3 * (size_t)t.tan.k * E), h->stream));     // acc, ke, umax (a failed call may leave them)
  // host memory: the control tangents and the mesh-sized outputs go through one device block of this call
  const size_t in_n = d_ext ? (size_t)K * T * mesh : d_actions ? (size_t)K * T * E * 2 * Mact : 0;
  const size_t hist_n = d_hist ? (size_t)K * T * 3 * E : 0, em_n = d_E_mesh ? (size_t)K * T * mesh : 0;
  const size_t kl_n = d_kl ? (size_t)K * T * E : 0, mom_n = d_moments ? (size_t)K * T * 3 * mesh : 0;
  const double* din = d_ext ? d_ext : d_actions;
  double* dhist = d_hist;
  double* dem = d_E_mesh;
  double* dkl = d_kl;
  double* dmom = d_moments;
  DeviceBuf<double> stage;
  if (host && in_n + hist_n + em_n + kl_n + mom_n > 0) {
    rc = regrow(h, stage, (in_n + hist_n + em_n + kl_n + mom_n) * sizeof(double), (w + ": the staging of host tangents does not fit on the device").c_str());
    if (rc) return rc;
    double* p = stage;
    HIPCHK(h, device_input(h, din, PIC_HOST, in_n * sizeof(double), p, &din));
    dhist = device_output(d_hist, PIC_HOST, p + in_n);
    dem = device_output(d_E_mesh, PIC_HOST, p + in_n + hist_n);
    dkl = device_output(d_kl, PIC_HOST, p + in_n + hist_n + em_n);
    dmom = device_output(d_moments, PIC_HOST, p + in_n + hist_n + em_n + kl_n);
  }
  rc = tangent_state_in(h, ta, d_x0, d_v0, mem_kind);
  if (rc) return rc;
  const AdjArgs a = adjoint_args(h);
  const WalkGeom g = walk_geom(h);
  hipLaunchKernelGGL(tangent_start_kernel, g.pgrid, dim3(ABLOCK), 0, h->stream, ta, a);
  ++t.launches;
  const TanGeom tg = tangent_geom(h, g, K);
  TanMeshIO io{};
  io.basis = h->basis; io.Mact = Mact;
  io.in_dstride = d_ext ? (long long)(T * mesh) : (long long)(T * E * 2 * Mact);
  io.out_hstride = (long long)(T * 3 * E); io.out_mstride = (long long)(T * mesh);
  const int64_t nseg = (T + t.every - 1) / t.every;
  for (int64_t sgi = 0; sgi < nseg; ++sgi) {
    rc = walk_replay(h, sgi, a, g);
    if (rc) return rc;
    const int64_t t0 = sgi * t.every, len = std::min<int64_t>(t.every, T - t0);
    for (int64_t i = 0; i < len; ++i) {
      const int64_t s = t0 + i;
      TanMeshIO m = io;
      m.ext = d_ext ? din + (size_t)s * mesh : nullptr;
      m.act = d_actions ? din + (size_t)s * E * 2 * Mact : nullptr;
      m.hist = dhist ? dhist + (size_t)s * 3 * E : nullptr;
      m.Emesh = dem ? dem + (size_t)s * mesh : nullptr;
      rc = tangent_step(h, ta, a, g, tg, i, m, dkl ? dkl + (size_t)s * E : nullptr, (long long)(T * E),
                        dmom ? dmom + (size_t)s * 3 * mesh : nullptr, (long long)(T * 3 * mesh));
      if (rc) return rc;
    }
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, device_result(h, d_hist, dhist, hist_n * sizeof(double)));
  HIPCHK(h, device_result(h, d_E_mesh, dem, em_n * sizeof(double)));
  HIPCHK(h, device_result(h, d_kl, dkl, kl_n * sizeof(double)));
  HIPCHK(h, device_result(h, d_moments, dmom, mom_n * sizeof(double)));
  rc = tangent_state_out(h, ta, mem_kind, d_x, d_v);
  return rc ? rc : walk_finish(h, w, mem_kind);
}

int pic_tape_tangent(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, const void* d_v0,
                     int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh) {
  if (!h) return PIC_EINVAL;
  return tape_tangent(h, "pic_tape_tangent", K, d_ext, d_actions, d_x0, d_v0, mem_kind, d_hist, d_x, d_v, d_E_mesh, nullptr);
}

int pic_tape_tangent_kl(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, const void* d_v0,
                        int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh, double* d_kl) {
  if (!h) return PIC_EINVAL;
  return tape_tangent(h, "pic_tape_tangent_kl", K, d_ext, d_actions, d_x0, d_v0, mem_kind, d_hist, d_x, d_v, d_E_mesh, d_kl);
}

int pic_tape_tangent_moments(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, const void* d_v0,
                             int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh, double* d_kl, double* d_moments) {
  if (!h) return PIC_EINVAL;
  return tape_tangent(h, d_moments ? "pic_tape_tangent_moments" : "pic_tape_tangent_kl", K, d_ext, d_actions, d_x0, d_v0, mem_kind,
                      d_hist, d_x, d_v, d_E_mesh, d_kl, d_moments);
}
