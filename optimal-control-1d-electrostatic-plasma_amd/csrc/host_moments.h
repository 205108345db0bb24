// host_moments.h -- included by picstep.hip alone, inside its extern "C" block and ahead of host_tape.h, whose walk calls
// tape_moments_reverse
#pragma once
// ---------------------------------------------------------------------------------------------
// Fluid moments on the mesh (include/picstep.h: pic_moments*, pic_tape_moments_cot; pic_moments.h)
// ---------------------------------------------------------------------------------------------
// the kernels' arguments and the deposit's grid: about 512 workgroups in all and at least 8192 particles each, so that the
// flush (up to 3 Ng memory-side atomics per workgroup) stays a small share of the pass
static MomArgs moments_args(const pic_handle* h, dim3& grid) {
  MomArgs a{};
  const long long N = h->cfg.N, E = h->cfg.num_envs;
  a.N = N; a.ld = h->ld; a.Ng = h->cfg.Ng; a.fg = h->fg; a.num_envs = (int)E; a.magic = h->magic;
  int b = 0;
  while (((int64_t)1 << b) < N) ++b;
  a.bitsN = b;
  a.L = h->cfg.L; a.dx = h->dx; a.scale = h->scale;
  const long long wpe = std::max(1LL, std::min((512 + E - 1) / E, (N + 8191) / 8192));
  const long long ntiles = (N + h->vec - 1) / h->vec;
  a.tiles_per_wg = (ntiles + wpe * BLOCK - 1) / (wpe * BLOCK);
  grid = dim3((unsigned)((ntiles + a.tiles_per_wg * BLOCK - 1) / (a.tiles_per_wg * BLOCK)), (unsigned)E);
  return a;
}

static size_t moments_lds(const pic_handle* h) { return (size_t)3 * (h->cfg.Ng + 2) * sizeof(unsigned long long); }

// the handle's block (host_blocks.h: moments_parts), allocated by the first call that needs it
static int moments_ensure(pic_handle* h, const char* who) {
  if (h->mom_block) return PIC_OK;
  if (moments_lds(h) > (size_t)(64 << 10))
    return fail(h, PIC_EINVAL, std::string(who) + ": N_mesh too large for three LDS meshes of 64-bit sums (at most 2728 cells)");
  const int rc = call_reserve(h, h->mom_block, nullptr, who, "the moments' accumulators", h->mom,
                              [&](Carver c, MomViews& v) { return moments_parts(c, block_dims(h), v); });
  if (rc) return rc;
  HIPCHK(h, hipMemsetAsync(h->mom.acc, 0, Carver::upto(h->mom.acc, h->mom.max + h->cfg.num_envs), h->stream));
  return PIC_OK;
}

// the three kernels of the moments of the handle's particles into m [env][3][Ng] (device memory), on the handle's stream
static hipError_t moments_enqueue(pic_handle* h, double* m) {
  dim3 grid;
  const MomArgs a = moments_args(h, grid);
  const size_t lds = moments_lds(h);
  const bool tsc = h->cfg.interpol == PIC_TSC;
  with_format(h, [&](auto p) {
    using P = decltype(p);
    const typename P::X* x = static_cast<const typename P::X*>(h->x.get());
    const typename P::V* v = static_cast<const typename P::V*>(h->v);
    hipLaunchKernelGGL((moments_max_kernel<P>), grid, dim3(BLOCK), 0, h->stream, v, h->mom.max, a);
    if (tsc)
      hipLaunchKernelGGL((moments_deposit_kernel<P, PIC_TSC>), grid, dim3(BLOCK), lds, h->stream, x, v,
                         (const unsigned long long*)h->mom.max, h->mom.acc, a);
    else
      hipLaunchKernelGGL((moments_deposit_kernel<P, PIC_CIC>), grid, dim3(BLOCK), lds, h->stream, x, v,
                         (const unsigned long long*)h->mom.max, h->mom.acc, a);
  });
  hipLaunchKernelGGL(moments_finish_kernel, dim3(h->cfg.num_envs), dim3(BLOCK), 0, h->stream, h->mom.acc, h->mom.max, m, a);
  return hipGetLastError();
}

int pic_moments(pic_handle* h, int mem_kind, double* m) {
  const char* who = "pic_moments";
  if (!h) return PIC_EINVAL;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (!m) return fail(h, PIC_EINVAL, std::string(who) + ": m is NULL");
  if (!h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, std::string(who) + ": a staged step is in progress");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (int rc = moments_ensure(h, who)) return rc;
  double* out = device_output(m, mem_kind, h->mom.out);
  hipError_t e = moments_enqueue(h, out);
  if (e == hipSuccess) e = device_result(h, m, out, (size_t)h->cfg.num_envs * 3 * h->cfg.Ng * sizeof(double));
  return hip_tail(h, e, mem_kind == PIC_HOST, who);      // device outputs stay stream-ordered
}

// the gather of a cotangent g [env][3][Ng] (device memory) at the particles x, v [env][ld] into rows of `orow` elements
// (overwritten, or added to)
static void moments_vjp_launch(pic_handle* h, bool add, const double* x, const double* v, const double* g, double* ox, double* ov,
                               long long orow) {
  dim3 unused;
  const MomArgs a = moments_args(h, unused);
  const dim3 grid((unsigned)((h->cfg.N + BLOCK - 1) / BLOCK), (unsigned)h->cfg.num_envs);
  if (add) hipLaunchKernelGGL(moments_vjp_kernel<true>, grid, dim3(BLOCK), 0, h->stream, x, v, g, a, ox, ov, orow);
  else hipLaunchKernelGGL(moments_vjp_kernel<false>, grid, dim3(BLOCK), 0, h->stream, x, v, g, a, ox, ov, orow);
}

int pic_moments_vjp(pic_handle* h, const double* cot_m, int mem_kind, void* g_x, void* g_v) {
  const char* who = "pic_moments_vjp";
  if (!h) return PIC_EINVAL;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (h->fmt != FMT_F64)
    return fail(h, PIC_EINVAL, std::string(who) + ": the gradient needs float64 particles with float64 positions (float32 and fixed32 "
                                                  "are not differentiated)");
  if (h->cfg.interpol != PIC_CIC)
    return fail(h, PIC_EINVAL, std::string(who) + ": the gradient needs CIC (the reference's TSC weights jump at cell edges: the "
                                                  "moments are not differentiable)");
  if (!cot_m) return fail(h, PIC_EINVAL, std::string(who) + ": cot_m is NULL");
  if (!h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, std::string(who) + ": a staged step is in progress");
  if (!g_x && !g_v) return PIC_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t E = h->cfg.num_envs, N = h->cfg.N, cbytes = E * 3 * h->cfg.Ng * sizeof(double), pbytes = E * N * sizeof(double);
  DeviceBuf<double> dcot, dgx, dgv;
  const double* cot = nullptr;
  const bool host = mem_kind == PIC_HOST;       // host memory goes through device buffers of this call, and so does a null output
  hipError_t e = hipSuccess;
  if (host) e = alloc(dcot, cbytes);
  if (e == hipSuccess) e = device_input(h, cot_m, mem_kind, cbytes, dcot, &cot);
  if (e == hipSuccess && (host || !g_x)) e = alloc(dgx, pbytes);
  if (e == hipSuccess && (host || !g_v)) e = alloc(dgv, pbytes);
  double* gx = g_x && !host ? static_cast<double*>(g_x) : dgx.get();
  double* gv = g_v && !host ? static_cast<double*>(g_v) : dgv.get();
  if (e == hipSuccess) {
    moments_vjp_launch(h, false, (const double*)h->x.get(), (const double*)h->v, cot, gx, gv, (long long)N);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = device_result(h, g_x, gx, pbytes);
  if (e == hipSuccess) e = device_result(h, g_v, gv, pbytes);
  return hip_tail(h, e, true, who);           // (this call's buffers go away behind it)
}

// ---------------------------------------------------------------------------------------------
// Cotangents on the moments of the states of a tape (hooks: walk_reverse, walk_close)
// ---------------------------------------------------------------------------------------------
// row s (-1: the start) of the open tape holds a cotangent
static bool tape_moments_row(const pic_handle* h, int64_t s) {
  const Tape& t = h->tape;
  return t.mom_cot.cot && t.mom_cot.flag[(size_t)(s + 1)];
}

// lambda += the gather of row s at the state x, v [env][ld] it belongs to (walk_reverse: the replayed state step s left;
// walk_close: the first checkpoint)
static void tape_moments_reverse(pic_handle* h, int64_t s, const double* x, const double* v, double* lx, double* lv) {
  Tape& t = h->tape;
  const double* g = t.mom_cot.cot + (size_t)(s + 1) * h->cfg.num_envs * 3 * h->cfg.Ng;
  moments_vjp_launch(h, true, x, v, g, lx, lv, (long long)h->ld);
  ++t.launches;
}

int pic_tape_moments_cot(pic_handle* h, const double* cot_m, int mem_kind, int64_t first_step, int64_t nsteps) {
  const char* who = "pic_tape_moments_cot";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (int rc = check_tape_open(h, who)) return rc;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (first_step < -1 || nsteps < 0 || first_step > t.steps || nsteps > t.steps - first_step)
    return fail(h, PIC_EINVAL, std::string(who) + ": rows outside the start (-1) and the " + std::to_string(t.steps) + " steps taped so far");
  if (nsteps == 0) return PIC_OK;
  if (t.walk.on && first_step + nsteps - 1 > t.walk.next)
    return fail(h, PIC_ESTATE, std::string(who) + ": the walk in progress has reversed step " + std::to_string(first_step + nsteps - 1) +
                                   " already");
  if (!t.mom_cot.cot) {
    if (!cot_m) return PIC_OK;                  // (no row was ever set: all are clear)
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const int rc = tape_reserve<MomCotViews>(h, t.mom_cot.block, who, "the moments' cotangents", t.mom_cot, [&](Carver c, MomCotViews& v) {
      return tape_moments_parts(c, block_dims(h), t.max_steps, v);
    });
    if (rc) return rc;
    t.mom_cot.flag.assign((size_t)t.max_steps + 1, 0);
  }
  if (cot_m) {
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const size_t row = (size_t)h->cfg.num_envs * 3 * h->cfg.Ng;
    HIPCHK(h, hipMemcpyAsync(t.mom_cot.cot + (size_t)(first_step + 1) * row, cot_m, (size_t)nsteps * row * sizeof(double),
                             copy_kind(mem_kind, hipMemcpyHostToDevice), h->stream));
    if (mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));      // (the caller's rows may go away behind this call)
  }
  std::fill(t.mom_cot.flag.begin() + (first_step + 1), t.mom_cot.flag.begin() + (first_step + 1 + nsteps), cot_m ? 1 : 0);
  return PIC_OK;
}

// ---------------------------------------------------------------------------------------------
// Forward mode of the moments (include/picstep.h: pic_moments_jvp, pic_tape_tangent_moments; pic_moments.h)
// ---------------------------------------------------------------------------------------------
// directions a deposit workgroup holds: three LDS meshes of Ng + 1 64-bit words each, within 64 KB (0: the mesh does not fit)
static int moments_jvp_kd(const pic_handle* h, int K) {
  return std::min<int>(K, (int)((size_t)(64 << 10) / ((size_t)3 * (h->cfg.Ng + 1) * sizeof(unsigned long long))));
}

// what pic_moments_jvp and the tape's tangent refuse alike
static int moments_jvp_check(pic_handle* h, const std::string& who) {
  if (h->fmt != FMT_F64)
    return fail(h, PIC_EINVAL, who + ": the tangent needs float64 particles with float64 positions (float32 and fixed32 are not "
                                     "differentiated)");
  if (h->cfg.interpol != PIC_CIC)
    return fail(h, PIC_EINVAL, who + ": the tangent needs CIC (the reference's TSC weights jump at cell edges: the moments are "
                                     "not differentiable)");
  if (moments_lds(h) > (size_t)(64 << 10))
    return fail(h, PIC_EINVAL, who + ": N_mesh too large for three LDS meshes of 64-bit sums (at most 2728 cells)");
  return PIC_OK;
}

// the three kernels: the moments' tangents at the particles x, v [env][ld] along the K directions of `j` (dx, dv, dstride, erow,
// acc, umax set by the caller) into out[d * out_dstride + (env 3 + m) Ng + node] (device memory), on the handle's stream
constexpr int kMomentsJvpLaunches = 3;
static hipError_t moments_jvp_enqueue(pic_handle* h, const double* x, const double* v, MomJvpArgs j, int K, double* out,
                                      long long out_dstride) {
  dim3 grid;
  const MomArgs a = moments_args(h, grid);
  j.K = K; j.kd = moments_jvp_kd(h, K);
  const dim3 dgrid(grid.x, grid.y, (unsigned)((K + j.kd - 1) / j.kd));
  const size_t lds = (size_t)j.kd * 3 * (h->cfg.Ng + 1) * sizeof(unsigned long long);
  if (K == 1) hipLaunchKernelGGL(moments_jvp_max_kernel<1>, grid, dim3(BLOCK), 0, h->stream, v, a, j);
  else if (K <= 4) hipLaunchKernelGGL(moments_jvp_max_kernel<4>, grid, dim3(BLOCK), 0, h->stream, v, a, j);
  else hipLaunchKernelGGL(moments_jvp_max_kernel<8>, grid, dim3(BLOCK), 0, h->stream, v, a, j);
  if (j.kd == 1) hipLaunchKernelGGL(moments_jvp_deposit_kernel<1>, dgrid, dim3(BLOCK), lds, h->stream, x, v, a, j);
  else if (j.kd <= 4) hipLaunchKernelGGL(moments_jvp_deposit_kernel<4>, dgrid, dim3(BLOCK), lds, h->stream, x, v, a, j);
  else hipLaunchKernelGGL(moments_jvp_deposit_kernel<8>, dgrid, dim3(BLOCK), lds, h->stream, x, v, a, j);
  hipLaunchKernelGGL(moments_jvp_finish_kernel, dim3(h->cfg.num_envs, K), dim3(BLOCK), 0, h->stream, a, j, out, out_dstride);
  return hipGetLastError();
}

int pic_moments_jvp(pic_handle* h, int K, const void* d_x, const void* d_v, int mem_kind, double* d_m) {
  const char* who = "pic_moments_jvp";
  if (!h) return PIC_EINVAL;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (int rc = moments_jvp_check(h, who)) return rc;
  if (K < 1 || K > kMaxTangents) return fail(h, PIC_EINVAL, std::string(who) + ": need 1 <= K <= " + std::to_string(kMaxTangents));
  if (!d_m) return fail(h, PIC_EINVAL, std::string(who) + ": d_m is NULL");
  if (!h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, std::string(who) + ": a staged step is in progress");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t E = h->cfg.num_envs, N = h->cfg.N, Ng = h->cfg.Ng;
  const size_t pbytes = (size_t)K * E * N * sizeof(double), obytes = (size_t)K * E * 3 * Ng * sizeof(double);
  MomJvpArgs j{};
  DeviceBuf<void> work;
  DeviceBuf<double> ddx, ddv, dout;
  const double *tx = nullptr, *tv = nullptr;
  const bool host = mem_kind == PIC_HOST;       // host memory goes through device buffers of this call
  // (a work block that does not fit has always been this entry's PIC_EHIP)
  hipError_t e = call_reserve(h, work, nullptr, who, "the working memory", j, [&](Carver c, MomJvpArgs& v) {
                   return moments_jvp_parts(c, block_dims(h), K, v);
                 }) ? hipErrorOutOfMemory : hipSuccess;
  if (e == hipSuccess) e = hipMemsetAsync(j.acc, 0, Carver::upto(j.acc, j.umax + (size_t)3 * K * E), h->stream);
  if (e == hipSuccess && host && d_x) e = alloc(ddx, pbytes);
  if (e == hipSuccess && host && d_v) e = alloc(ddv, pbytes);
  if (e == hipSuccess) e = device_input(h, static_cast<const double*>(d_x), mem_kind, pbytes, ddx, &tx);
  if (e == hipSuccess) e = device_input(h, static_cast<const double*>(d_v), mem_kind, pbytes, ddv, &tv);
  if (e == hipSuccess && host) e = alloc(dout, obytes);
  double* out = device_output(d_m, mem_kind, dout);
  if (e == hipSuccess) {
    j.dx = tx; j.dv = tv; j.dstride = (long long)(E * N); j.erow = (long long)N;
    e = moments_jvp_enqueue(h, (const double*)h->x.get(), (const double*)h->v, j, K, out, (long long)(E * 3 * Ng));
  }
  if (e == hipSuccess) e = device_result(h, d_m, out, obytes);
  return hip_tail(h, e, true, who);           // (this call's buffers go away behind it)
}

// ---------------------------------------------------------------------------------------------
// The moments of every taped step (include/picstep.h: pic_tape_moments_start, pic_tape_moments; hook: advance)
// ---------------------------------------------------------------------------------------------
int pic_tape_moments_start(pic_handle* h) {
  const char* who = "pic_tape_moments_start";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (int rc = check_tape_open(h, who)) return rc;
  if (t.mom_trace.trace) return fail(h, PIC_ESTATE, std::string(who) + ": the tape has a moments trace already");
  if (t.steps != 0) return fail(h, PIC_ESTATE, std::string(who) + ": the tape holds steps already (start the trace before the first)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int rc = tape_reserve<MomTraceViews>(h, t.mom_trace.block, who, "the moments' trace", t.mom_trace, [&](Carver c, MomTraceViews& v) {
    return tape_moments_trace_parts(c, block_dims(h), t.max_steps, v);
  });
  if (!rc && (rc = moments_ensure(h, who)) != PIC_OK) tape_release(t, t.mom_trace);      // (budget_bytes first, then what allocates)
  return rc;
}

// the moments of the handle's particles into row t.steps of the trace (advance, behind the step that is about to be counted)
static int tape_moments_enqueue(pic_handle* h) {
  Tape& t = h->tape;
  HIPCHK(h, moments_enqueue(h, t.mom_trace.trace + (size_t)t.steps * h->cfg.num_envs * 3 * h->cfg.Ng));
  return PIC_OK;
}

int pic_tape_moments(pic_handle* h, int mem_kind, double* m) {
  const char* who = "pic_tape_moments";
  if (!h) return PIC_EINVAL;
  Tape& t = h->tape;
  if (!t.on || !t.mom_trace.trace)
    return fail(h, PIC_ESTATE, std::string(who) + ": no tape with a moments trace is open (pic_tape_moments_start)");
  if ((mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) || !m) return fail(h, PIC_EINVAL, std::string(who) + ": bad mem_kind or null m");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (t.steps == 0) return PIC_OK;
  HIPCHK(h, hipMemcpyAsync(m, t.mom_trace.trace, (size_t)t.steps * h->cfg.num_envs * 3 * h->cfg.Ng * sizeof(double),
                           copy_kind(mem_kind, hipMemcpyDeviceToHost), h->stream));
  if (mem_kind == PIC_HOST) HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIC_OK;
}
