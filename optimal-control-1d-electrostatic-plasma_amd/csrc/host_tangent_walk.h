// host_tangent_walk.h -- included by picstep.hip alone, inside its extern "C" block, behind host_tangent.h (tangent_step is the walk's)
#pragma once
// ---------------------------------------------------------------------------------------------
// Forward mode through closed loops (include/picstep.h: pic_tape_tangent_walk_*, pic_tape_tangent_feedback; kernels: pic_tangent.h;
// DESIGN.md 7n): the tape's steps one at a time, forward in time, with the action tangent of a step fed from the field tangent
// the step before left -- by the gain law on the device, by the caller between two steps, or (pic_tape_tangent_policy, DESIGN.md
// 7q) by the MLP policy's JVP kernel on the device
// ---------------------------------------------------------------------------------------------
// the walk's working rows (host_blocks.h: tanwalk_parts) for K directions and mo modes, within budget_bytes (grown for more; on
// failure the tape keeps what it had)
static int tanwalk_reserve(pic_handle* h, int K, int mo, const char* who) {
  Tape::TanWalk& w = h->tape.twalk;
  if (w.cap_k >= K && w.cap_mo >= mo && w.block) return PIC_OK;
  const int kc = std::max(K, w.cap_k), mc = std::max(mo, w.cap_mo);
  const int rc = tape_reserve<TanWalkViews>(h, w.block, who, "the walk's working rows", w,
                                            [&](Carver c, TanWalkViews& v) { return tanwalk_parts(c, block_dims(h), kc, mc, v); });
  if (!rc) { w.cap_k = kc; w.cap_mo = mc; }
  return rc;
}

// the working rows of a walk through the policy's steps (host_blocks.h: tanpol_parts) for K directions, likewise
static int tanpol_reserve(pic_handle* h, int K, const char* who) {
  Tape& t = h->tape;
  if (t.tpol.cap_k >= K && t.tpol.block) return PIC_OK;
  BlockDims d = block_dims(h);        // (with what the tape keeps of its policy: the layout reads no more of it)
  d.P = t.policy.P; d.per_env = t.policy.shape.per_env != 0;
  const int rc = tape_reserve<TanPolViews>(h, t.tpol.block, who, "the policy tangent's working rows", t.tpol,
                                           [&](Carver c, TanPolViews& v) { return tanpol_parts(c, d, K, v); });
  if (!rc) t.tpol.cap_k = K;
  return rc;
}

// the modes the gain law of this tape reads (0: no law step was taped)
static int tanwalk_law_modes(const pic_handle* h) { return h->tape.law.act ? h->act_modes : 0; }

// K rows of n doubles from the walk's contiguous rows to the caller's array in mem_kind's memory, its rows `pitch` doubles apart
static hipError_t tanwalk_rows_out(pic_handle* h, double* dst, size_t pitch, const double* src, size_t n, int K, int mem_kind) {
  if (!dst || !n) return hipSuccess;
  const hipMemcpyKind kind = copy_kind(mem_kind, hipMemcpyDeviceToHost);
  if (pitch == n) return hipMemcpyAsync(dst, src, (size_t)K * n * sizeof(double), kind, h->stream);
  return hipMemcpy2DAsync(dst, pitch * sizeof(double), src, n * sizeof(double), n * sizeof(double), (size_t)K, kind, h->stream);
}

static hipError_t tanwalk_rows_zero(pic_handle* h, double* dst, size_t pitch, size_t n, int K, int mem_kind) {
  if (!dst || !n) return hipSuccess;
  if (mem_kind == PIC_HOST) {
    for (int d = 0; d < K; ++d) std::memset(dst + (size_t)d * pitch, 0, n * sizeof(double));
    return hipSuccess;
  }
  return hipMemset2DAsync(dst, pitch * sizeof(double), 0, n * sizeof(double), (size_t)K, h->stream);
}

// dm = J dM of the field tangent in v.dM (the field step s_next reads): the observation's tangent, the law's dm, and the da row of
// step s_next if it is a law step (pic_tangent.h: tangent_law_kernel).  Nothing to do without a law block and an observation.
static void tanwalk_law(pic_handle* h, const TanWalkViews& v, int64_t s_next) {
  Tape& t = h->tape;
  const int Ml = tanwalk_law_modes(h), mo = t.twalk.mo, E = h->cfg.num_envs;
  if (Ml == 0 && mo == 0) return;
  const bool lawstep = tape_law_step(h, s_next);
  TanLawArgs l{};
  l.dM = v.dM; l.tw = (const double*)h->tw; l.rows = h->tw_rows;
  l.obs = mo ? v.obs : nullptr;
  l.dm = v.dm;
  l.gain = lawstep ? (const double*)t.law.gains[(size_t)t.law.step[(size_t)s_next]] : nullptr;
  l.dgain = lawstep && t.twalk.dgain ? v.dG : nullptr;
  l.modes = lawstep ? t.law.modes + (size_t)s_next * E * 2 * Ml : nullptr;
  l.da = v.da;
  l.Ng = h->cfg.Ng; l.M = Ml; l.Mo = mo; l.num_envs = E;
  hipLaunchKernelGGL(tangent_law_kernel, dim3(E, t.twalk.k), dim3(ABLOCK), 0, h->stream, l);
  ++t.launches;
}

extern "C++" {
static void tangent_start_deposit(pic_handle* h, const double* x, const TanArgs& ta, const AdjArgs& a, const TanGeom& tg) {
  if (tg.kd == 1) hipLaunchKernelGGL((tangent_start_deposit_kernel<1>), tg.dgrid, dim3(ABLOCK), tg.dlds, h->stream, x, ta, a, tg.kd);
  else if (tg.kd <= 4) hipLaunchKernelGGL((tangent_start_deposit_kernel<4>), tg.dgrid, dim3(ABLOCK), tg.dlds, h->stream, x, ta, a, tg.kd);
  else hipLaunchKernelGGL((tangent_start_deposit_kernel<8>), tg.dgrid, dim3(ABLOCK), tg.dlds, h->stream, x, ta, a, tg.kd);
}
}  // extern "C++"

// pic_tape_tangent_walk_begin, the start of pic_tape_tangent_feedback (mo = 0) and, with `policy`, of pic_tape_tangent_policy
// (mo = the policy's M_o; d_params [K][P] or [K][env][P], null = 0): only that one goes through the steps of pic_tape_step_policy
static int tanwalk_open(pic_handle* h, const char* who, int K, int mo, const void* d_x0, const void* d_v0, const double* d_gain,
                        int mem_kind, double* d_modes0, bool policy = false, const double* d_params = nullptr) {
  Tape& t = h->tape;
  const std::string w(who);
  if (int rc = check_tape_open(h, who)) return rc;
  if (!policy)
    if (int rc = check_no_policy_steps(h, who)) return rc;
  if (K < 1 || K > kMaxTangents) return fail(h, PIC_EINVAL, w + ": need 1 <= K <= " + std::to_string(kMaxTangents));
  if (mo < 0 || mo >= h->cfg.Ng) return fail(h, PIC_EINVAL, w + ": need obs_modes = 0 or 1 <= obs_modes < N_mesh");
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (d_modes0 && mo == 0) return fail(h, PIC_EINVAL, w + ": d_modes0 needs obs_modes >= 1");
  const int64_t T = t.steps;
  bool law = false;
  for (int64_t s = 0; s < T && !law; ++s) law = tape_law_step(h, s);
  if (d_gain && !law) return fail(h, PIC_EINVAL, w + ": d_gain needs a step of pic_step_feedback_gain on the tape");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  t.walk.on = t.twalk.on = false;           // (a walk's replayed segment is about to be overwritten)
  const int E = h->cfg.num_envs, Ng = h->cfg.Ng, Ml = tanwalk_law_modes(h);
  const size_t mesh = (size_t)E * Ng, arow = (size_t)E * 2 * h->act_modes;
  int rc = std::max(Ml, mo) > 0 ? ensure_twiddle(h, std::max(Ml, mo)) : PIC_OK;
  if (!rc) rc = tangent_reserve(h, K, who);
  if (!rc) rc = tanwalk_reserve(h, K, mo, who);
  if (!rc && policy) rc = tanpol_reserve(h, K, who);
  if (rc) return rc;
  t.launches = 0;
  HIPCHK(h, hipMemsetAsync(t.counters, 0, 2 * sizeof(unsigned long long), h->stream));
  const TanArgs ta = tangent_args(h, K);
  const TanWalkViews& v = t.twalk;
  HIPCHK(h, hipMemsetAsync(ta.acc, 0, Carver::upto(ta.acc, ta.umax + 3 * (size_t)t.tan.k * E), h->stream));     // acc, ke, umax
  rc = tangent_state_in(h, ta, d_x0, d_v0, mem_kind);
  if (rc) return rc;
  if (d_gain) HIPCHK(h, device_fill(h, v.dG, d_gain, (size_t)K * arow * 2 * h->act_modes * sizeof(double), mem_kind));
  t.twalk.k = K; t.twalk.mo = mo; t.twalk.dgain = d_gain != nullptr;
  t.twalk.policy = policy; t.tpol.dparams = policy && d_params;
  if (t.tpol.dparams)
    HIPCHK(h, device_fill(h, t.tpol.dtheta, d_params, (size_t)K * (t.policy.shape.per_env ? E : 1) * t.policy.P * sizeof(double), mem_kind));
  const AdjArgs a = adjoint_args(h);
  const WalkGeom g = walk_geom(h);
  if (Ml > 0 || mo > 0) {
    // the tangent of the field the tape started from, dE_0 = K drho(x_0; dx_0), read by the observation o_0 and by a first law step
    const TanGeom tg = tangent_geom(h, g, K);
    if (d_x0) {
      hipLaunchKernelGGL(tangent_x_max_kernel, g.pgrid, dim3(ABLOCK), 0, h->stream, ta, a);
      tangent_start_deposit(h, t.ck, ta, a, tg);
      t.launches += 2;
    }
    HIPCHK(h, hipMemsetAsync(ta.dF, 0, mesh * sizeof(double), h->stream));      // stands in for a post-step field: no energies here
    TanMeshIO m{};
    m.basis = h->basis; m.Mact = h->act_modes;
    m.M = ta.dF; m.Emesh = v.dM; m.out_mstride = (long long)mesh;
    hipLaunchKernelGGL(tangent_mesh_kernel<4>, tg.mgrid, dim3(SBLOCK), g.mesh_lds, h->stream, ta, m, a);
    ++t.launches;
    tanwalk_law(h, v, 0);
  }
  hipLaunchKernelGGL(tangent_start_kernel, g.pgrid, dim3(ABLOCK), 0, h->stream, ta, a);
  ++t.launches;
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, tanwalk_rows_out(h, d_modes0, (size_t)E * 2 * mo, v.obs, (size_t)E * 2 * mo, K, mem_kind));
  if (d_modes0 && mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  t.twalk.on = true;
  t.twalk.next = 0;
  return PIC_OK;
}

// what a step of the walk takes and returns, in mem_kind's memory: every array's direction d lies d * its pitch doubles behind
// direction 0's row (the walk: one step's arrays; pic_tape_tangent_feedback: rows of the whole trajectory's)
struct TanWalkIO {
  const double* ext = nullptr;        // [env][Ng]
  const double* act = nullptr;        // [env][2M]
  const double* pre = nullptr;        // [env][2M] added to du on a policy step (pic_tape_tangent_policy); act's pitch
  size_t in_pitch = 0;
  double* hist = nullptr;             // [3][env]
  size_t hist_pitch = 0;
  double* obs = nullptr;              // [env][2 Mo] of the field the step left; contiguous directions
  double* lawm = nullptr;             // [env][2M] the law's dm of the field the step read (zero on other steps)
  double* aout = nullptr;             // [env][2M] the action tangent applied
  double* uout = nullptr;             // [env][2M] du of a policy step (zero on other steps)
  size_t act_pitch = 0;               // of lawm, aout and uout
  double* obs_in = nullptr;           // [env][2 Mo] the observation's tangent of the field the step read
  size_t obs_pitch = 0;
  double* em = nullptr;               // [env][Ng]
  size_t em_pitch = 0;
};

// step t.twalk.next of a live walk: first the replay of its segment if it is the segment's first step
static int tanwalk_advance(pic_handle* h, const TanWalkIO& io, int mem_kind) {
  Tape& t = h->tape;
  const int E = h->cfg.num_envs, K = t.twalk.k, Mact = h->act_modes;
  const size_t mesh = (size_t)E * h->cfg.Ng, arow = (size_t)E * 2 * Mact;
  const int64_t s = t.twalk.next, sgi = s / t.every, i = s - sgi * t.every;
  const AdjArgs a = adjoint_args(h);
  const WalkGeom g = walk_geom(h);
  const TanGeom tg = tangent_geom(h, g, K);
  const TanArgs ta = tangent_args(h, K);
  const TanWalkViews& v = t.twalk;
  const bool lawstep = tape_law_step(h, s), polstep = t.twalk.policy && tape_policy_step(h, s), host = mem_kind == PIC_HOST;
  if (i == 0)
    if (int rc = walk_replay(h, sgi, a, g)) return rc;
  if (io.lawm) HIPCHK(h, lawstep ? tanwalk_rows_out(h, io.lawm, io.act_pitch, v.dm, arow, K, mem_kind)
                                 : tanwalk_rows_zero(h, io.lawm, io.act_pitch, arow, K, mem_kind));
  TanMeshIO m{};
  m.basis = h->basis; m.Mact = Mact;
  m.hist = io.hist ? v.hist : nullptr; m.out_hstride = (long long)(3 * E);
  m.Emesh = v.dM; m.out_mstride = (long long)mesh;
  // the injection: device memory is read where it lies, host memory through the walk's row
  const double* in = io.ext ? io.ext : io.act;
  size_t in_pitch = io.in_pitch;
  if (in && host) {
    const size_t n = io.ext ? mesh : arow;
    HIPCHK(h, hipMemcpy2DAsync(v.in, n * sizeof(double), in, in_pitch * sizeof(double), n * sizeof(double), (size_t)K, hipMemcpyHostToDevice,
                               h->stream));
    in = v.in;
    in_pitch = n;
  }
  HIPCHK(h, tanwalk_rows_out(h, io.obs_in, io.obs_pitch, v.obs, (size_t)E * 2 * t.twalk.mo, K, mem_kind));
  if (polstep) {                        // da_s = the policy's JVP at (o_s, u_s) along (dtheta, do_s, d_pre_s), + the caller's
    const TanPolViews& pv = t.tpol;
    const Tape::Policy::Copy& pc = t.policy.calls[(size_t)t.policy.step[(size_t)s]];
    const size_t orow = (size_t)E * 2 * t.policy.shape.obs_modes;
    const double* pre = io.pre;
    size_t pre_pitch = io.in_pitch;
    if (pre && host) {
      HIPCHK(h, hipMemcpy2DAsync(pv.pin, arow * sizeof(double), pre, pre_pitch * sizeof(double), arow * sizeof(double), (size_t)K,
                                 hipMemcpyHostToDevice, h->stream));
      pre = pv.pin;
      pre_pitch = arow;
    }
    PolicyJvpArgs pa{};
    pa.obs = t.policy.obs + (size_t)s * orow;
    pa.obs_scale = pc.scale;
    pa.params = pc.params.get();
    pa.pre = t.policy.pre + (size_t)s * arow;
    pa.d_params = t.tpol.dparams ? pv.dtheta : nullptr;
    pa.d_obs = v.obs;
    pa.d_pre = pre;
    pa.d_act = in;
    pa.du = pv.du;
    pa.da = v.da;
    pa.dparams_stride = (long long)((t.policy.shape.per_env ? (size_t)E : 1) * t.policy.P);
    pa.dobs_stride = (long long)orow;
    pa.dpre_stride = (long long)pre_pitch;
    pa.dact_stride = (long long)in_pitch;
    pa.du_stride = pa.da_stride = (long long)arow;
    policy_shape(pa, t.policy.shape, t.policy.P, pc.action_scale);
    hipLaunchKernelGGL(policy_jvp_kernel, dim3(E, K), dim3(BLOCK), 0, h->stream, pa);
    ++t.launches;
    m.act = v.da; m.in_dstride = (long long)arow;
  } else if (io.ext) {
    m.ext = in; m.in_dstride = (long long)in_pitch;
  } else if (io.act || lawstep) {
    if (io.act) {                     // da_s = (G dm + dG m) + the caller's, or the caller's alone
      hipLaunchKernelGGL(tangent_action_kernel, dim3((unsigned)((arow + ABLOCK - 1) / ABLOCK), K), dim3(ABLOCK), 0, h->stream, v.da, in,
                         (long long)in_pitch, (int)arow, lawstep ? 1 : 0);
      ++t.launches;
    }
    m.act = v.da; m.in_dstride = (long long)arow;
  }
  if (io.aout) HIPCHK(h, m.act ? tanwalk_rows_out(h, io.aout, io.act_pitch, v.da, arow, K, mem_kind)
                               : tanwalk_rows_zero(h, io.aout, io.act_pitch, arow, K, mem_kind));
  if (io.uout) HIPCHK(h, polstep ? tanwalk_rows_out(h, io.uout, io.act_pitch, t.tpol.du, arow, K, mem_kind)
                                 : tanwalk_rows_zero(h, io.uout, io.act_pitch, arow, K, mem_kind));
  if (int rc = tangent_step(h, ta, a, g, tg, i, m, nullptr, 0, nullptr, 0)) return rc;
  tanwalk_law(h, v, s + 1);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, tanwalk_rows_out(h, io.hist, io.hist_pitch, v.hist, (size_t)3 * E, K, mem_kind));
  HIPCHK(h, tanwalk_rows_out(h, io.obs, (size_t)E * 2 * t.twalk.mo, v.obs, (size_t)E * 2 * t.twalk.mo, K, mem_kind));
  HIPCHK(h, tanwalk_rows_out(h, io.em, io.em_pitch, v.dM, mesh, K, mem_kind));
  ++t.twalk.next;
  return PIC_OK;
}

int pic_tape_tangent_walk_begin(pic_handle* h, int K, int obs_modes, const void* d_x0, const void* d_v0, const double* d_gain,
                                int mem_kind, double* d_modes0) {
  if (!h) return PIC_EINVAL;
  return tanwalk_open(h, "pic_tape_tangent_walk_begin", K, obs_modes, d_x0, d_v0, d_gain, mem_kind, d_modes0);
}

int pic_tape_tangent_walk_step(pic_handle* h, const double* d_ext, const double* d_actions, int mem_kind, double* d_energies,
                               double* d_modes, double* d_actions_out, void* d_x, void* d_v, double* d_E_mesh, int64_t* step) {
  const char* who = "pic_tape_tangent_walk_step";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.twalk.on) return fail(h, PIC_ESTATE, std::string(who) + ": no tangent walk in progress (pic_tape_tangent_walk_begin)");
  if (t.twalk.next >= t.steps) return fail(h, PIC_ESTATE, std::string(who) + ": every step has been walked (pic_tape_tangent_walk_end)");
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (d_ext && d_actions) return fail(h, PIC_EINVAL, std::string(who) + ": d_ext and d_actions are both given (at most one)");
  if (d_ext && tape_law_step(h, t.twalk.next))
    return fail(h, PIC_EINVAL, std::string(who) + ": d_ext on a step of pic_step_feedback_gain (inject through d_actions)");
  if (d_modes && t.twalk.mo == 0) return fail(h, PIC_EINVAL, std::string(who) + ": d_modes needs a walk begun with obs_modes >= 1");
  if (int rc = check_tape_actuator(h, d_actions, "d_actions", who)) return rc;
  if (int rc = check_tape_actuator(h, d_actions_out, "d_actions_out", who)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t E = h->cfg.num_envs, mesh = E * h->cfg.Ng, arow = E * 2 * h->act_modes;
  TanWalkIO io;
  io.ext = d_ext; io.act = d_actions; io.in_pitch = d_ext ? mesh : arow;
  io.hist = d_energies; io.hist_pitch = 3 * E;
  io.obs = d_modes;
  io.aout = d_actions_out; io.act_pitch = arow;
  io.em = d_E_mesh; io.em_pitch = mesh;
  const int64_t s = t.twalk.next;
  int rc = tanwalk_advance(h, io, mem_kind);
  if (!rc) rc = tangent_state_out(h, tangent_args(h, t.twalk.k), mem_kind, d_x, d_v);
  if (rc) { t.twalk.on = false; return rc; }
  if (mem_kind == PIC_HOST && (d_energies || d_modes || d_actions_out || d_x || d_v || d_E_mesh)) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (step) *step = s;
  return PIC_OK;
}

int pic_tape_tangent_walk_end(pic_handle* h, int mem_kind, void* d_x, void* d_v) {
  const char* who = "pic_tape_tangent_walk_end";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.twalk.on) return fail(h, PIC_ESTATE, std::string(who) + ": no tangent walk in progress (pic_tape_tangent_walk_begin)");
  if (t.twalk.next < t.steps)
    return fail(h, PIC_ESTATE, std::string(who) + ": " + std::to_string(t.steps - t.twalk.next) + " steps are not walked yet (pic_tape_tangent_walk_step)");
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  t.twalk.on = false;
  const int rc = tangent_state_out(h, tangent_args(h, t.twalk.k), mem_kind, d_x, d_v);
  return rc ? rc : walk_finish(h, who, mem_kind);
}

int pic_tape_tangent_feedback(pic_handle* h, int K, const double* d_gain, const void* d_x0, const void* d_v0, const double* d_actions,
                              int mem_kind, double* d_hist, double* d_modes, double* d_actions_out, void* d_x, void* d_v,
                              double* d_E_mesh) {
  const char* who = "pic_tape_tangent_feedback";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (int rc = check_tape_open(h, who)) return rc;
  if (int rc = check_no_policy_steps(h, who)) return rc;
  for (const void* p : {(const void*)d_actions, (const void*)d_modes, (const void*)d_actions_out})
    if (int rc = check_tape_actuator(h, p, "d_actions, d_modes or d_actions_out", who)) return rc;
  int rc = tanwalk_open(h, who, K, 0, d_x0, d_v0, d_gain, mem_kind, nullptr);
  if (rc) return rc;
  const size_t E = h->cfg.num_envs, mesh = E * h->cfg.Ng, arow = E * 2 * h->act_modes, T = (size_t)t.steps;
  for (size_t s = 0; s < T; ++s) {
    TanWalkIO io;
    io.act = d_actions ? d_actions + s * arow : nullptr; io.in_pitch = T * arow;
    io.hist = d_hist ? d_hist + s * 3 * E : nullptr; io.hist_pitch = T * 3 * E;
    io.lawm = d_modes ? d_modes + s * arow : nullptr;
    io.aout = d_actions_out ? d_actions_out + s * arow : nullptr; io.act_pitch = T * arow;
    io.em = d_E_mesh ? d_E_mesh + s * mesh : nullptr; io.em_pitch = T * mesh;
    rc = tanwalk_advance(h, io, mem_kind);
    if (rc) { t.twalk.on = false; return rc; }
  }
  t.twalk.on = false;
  rc = tangent_state_out(h, tangent_args(h, t.twalk.k), mem_kind, d_x, d_v);
  return rc ? rc : walk_finish(h, who, mem_kind);
}

int pic_tape_tangent_policy(pic_handle* h, int K, const double* d_params, const double* d_pre, const double* d_actions, const void* d_x0,
                            const void* d_v0, int mem_kind, double* d_hist, double* d_obs, double* d_pre_out, double* d_actions_out,
                            void* d_x, void* d_v, double* d_E_mesh) {
  const char* who = "pic_tape_tangent_policy";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (int rc = check_tape_open(h, who)) return rc;
  if (!t.policy.block) return fail(h, PIC_EINVAL, std::string(who) + ": the tape holds no steps of pic_tape_step_policy");
  const int mo = t.policy.shape.obs_modes;
  int rc = tanwalk_open(h, who, K, mo, d_x0, d_v0, nullptr, mem_kind, nullptr, true, d_params);
  if (rc) return rc;
  const size_t E = h->cfg.num_envs, mesh = E * h->cfg.Ng, arow = E * 2 * h->act_modes, orow = E * 2 * mo, T = (size_t)t.steps;
  for (size_t s = 0; s < T; ++s) {
    TanWalkIO io;
    io.act = d_actions ? d_actions + s * arow : nullptr; io.in_pitch = T * arow;
    io.pre = d_pre ? d_pre + s * arow : nullptr;
    io.hist = d_hist ? d_hist + s * 3 * E : nullptr; io.hist_pitch = T * 3 * E;
    io.obs_in = d_obs ? d_obs + s * orow : nullptr; io.obs_pitch = T * orow;
    io.uout = d_pre_out ? d_pre_out + s * arow : nullptr;
    io.aout = d_actions_out ? d_actions_out + s * arow : nullptr; io.act_pitch = T * arow;
    io.em = d_E_mesh ? d_E_mesh + s * mesh : nullptr; io.em_pitch = T * mesh;
    rc = tanwalk_advance(h, io, mem_kind);
    if (rc) { t.twalk.on = false; return rc; }
  }
  t.twalk.on = false;
  rc = tangent_state_out(h, tangent_args(h, t.twalk.k), mem_kind, d_x, d_v);
  return rc ? rc : walk_finish(h, who, mem_kind);
}
