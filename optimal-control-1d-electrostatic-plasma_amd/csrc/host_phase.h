// host_phase.h -- included by picstep.hip alone, inside its extern "C" block
#pragma once
// ---------------------------------------------------------------------------------------------
// Smoothed phase-space density and KL (include/picstep.h: pic_phase_kl_smooth*; pic_phase.h)
// ---------------------------------------------------------------------------------------------
static int phase_check(pic_handle* h, const pic_phase_spec* s, int mem_kind, const char* who) {
  if (!h) return PIC_EINVAL;
  const std::string w(who);
  if (!s || s->nx < 1 || s->nx > kPhaseMaxBins || s->nv < 1 || s->nv > kPhaseMaxBins ||
      !(std::isfinite(s->vmin) && std::isfinite(s->vmax) && s->vmax > s->vmin))
    return fail(h, PIC_EINVAL, w + ": need a spec with 1 <= nx, nv <= 1024 and finite vmin < vmax");
  if ((mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) ||
      (s->feq && s->feq_mem_kind != PIC_HOST && s->feq_mem_kind != PIC_DEVICE))
    return fail(h, PIC_EINVAL, w + ": mem_kind must be PIC_HOST or PIC_DEVICE");
  if (h->fmt != FMT_F64) return fail(h, PIC_EINVAL, w + ": float64 particles and positions only");
  if (!h->has_state) return fail(h, PIC_ESTATE, w + ": call pic_reset first");
  return PIC_OK;
}

// the density's normalisation n0 / dx / dv / N of a spec's bins (objective.py:12, left to right)
static double phase_norm(const pic_handle* h, const pic_phase_spec* s) {
  const double dx = h->cfg.L / s->nx, dv = (s->vmax - s->vmin) / s->nv;
  return h->cfg.n0 / dx / dv / (double)h->cfg.N;
}

static PhaseArgs phase_args(const pic_handle* h, const pic_phase_spec* s, dim3& grid) {
  PhaseArgs a{};
  const long long N = h->cfg.N;
  a.N = N; a.ld = h->ld; a.nx = s->nx; a.nv = s->nv;
  a.rows = std::min(s->nx, std::max(1, kPhaseLdsBytes / (8 * s->nv)));
  int bitsN = 1;                                     // N < 2^bitsN: N particles of 2^(62 - bitsN) units stay below 2^62
  while (bitsN < 62 && (N >> bitsN) != 0) ++bitsN;
  const int su = 62 - bitsN;
  a.abits = (su + 1) / 2; a.bbits = su / 2;
  a.L = h->cfg.L; a.vmin = s->vmin; a.vmax = s->vmax;
  a.rdx = 1.0 / (h->cfg.L / s->nx);
  a.rdv = 1.0 / ((s->vmax - s->vmin) / s->nv);
  // A band's workgroups each flush up to rows * nv words: few workgroups per (environment, band) with long particle ranges
  // (about 512 workgroups in all, at least 8192 particles each) keep the flush a small share of the pass.
  const int bands = (s->nx + a.rows - 1) / a.rows;
  const long long per = (long long)bands * h->cfg.num_envs;
  const long long wpe = std::max(1LL, std::min((512 + per - 1) / per, (N + 8191) / 8192));
  const long long ntiles = (N + 1) / 2;
  a.tiles_per_wg = (ntiles + wpe * BLOCK - 1) / (wpe * BLOCK);
  grid = dim3((unsigned)((ntiles + a.tiles_per_wg * BLOCK - 1) / (a.tiles_per_wg * BLOCK)), (unsigned)bands,
              (unsigned)h->cfg.num_envs);
  return a;
}

// The deposit of the particles x, v [env][ld] (the handle's, or a replayed state of the tape) and the finishing kernel behind
// it, on the handle's stream.  acc: [env][nx][nv] zero (left zero); feq: device memory or null; d_kl, f, kl, g: device memory or
// null (PhaseFinishArgs).
static hipError_t phase_enqueue(pic_handle* h, const pic_phase_spec* s, const double* x, const double* v, unsigned long long* acc,
                                const double* feq, const double* d_kl, double* f, double* kl, double* g, PhaseArgs& a) {
  dim3 grid;
  a = phase_args(h, s, grid);
  hipLaunchKernelGGL(phase_deposit_kernel, grid, dim3(BLOCK), (size_t)a.rows * a.nv * sizeof(unsigned long long), h->stream,
                     x, v, acc, a);
  const double dx = h->cfg.L / s->nx, dv = (s->vmax - s->vmin) / s->nv;
  PhaseFinishArgs fa{};
  fa.acc = acc; fa.nb2 = s->nx * s->nv;
  fa.unit = ldexp(1.0, -(a.abits + a.bbits));
  fa.norm = phase_norm(h, s);
  fa.dxdv = dx * dv;
  fa.feq = feq; fa.feq_stride = s->feq_per_env ? fa.nb2 : 0;
  fa.d_kl = d_kl; fa.f = f; fa.kl = kl; fa.g = g;
  hipLaunchKernelGGL(phase_finish_kernel, dim3(h->cfg.num_envs), dim3(BLOCK), 0, h->stream, fa);
  return hipGetLastError();
}

int pic_phase_kl_smooth(pic_handle* h, const pic_phase_spec* s, int mem_kind, double* kl, double* f) {
  int rc = phase_check(h, s, mem_kind, "pic_phase_kl_smooth");
  if (rc) return rc;
  if (!kl && !f) return fail(h, PIC_EINVAL, "pic_phase_kl_smooth: kl and f are both NULL");
  if (kl && !s->feq) return fail(h, PIC_EINVAL, "pic_phase_kl_smooth: kl needs spec->feq");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs;
  const size_t nb2 = (size_t)s->nx * s->nv, feq_bytes = (s->feq_per_env ? E : 1) * nb2 * sizeof(double);
  DeviceBuf<unsigned long long> acc;
  DeviceBuf<double> dfeq, df, dkl;
  const double* feq = nullptr;
  PhaseArgs a;
  const bool host = mem_kind == PIC_HOST;       // host memory goes through device buffers of this call
  hipError_t e = alloc_zeroed(acc, (size_t)E * nb2 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess && s->feq && s->feq_mem_kind == PIC_HOST) e = alloc(dfeq, feq_bytes);
  if (e == hipSuccess) e = device_input(h, s->feq, s->feq_mem_kind, feq_bytes, dfeq, &feq);
  if (e == hipSuccess && f && host) e = alloc(df, (size_t)E * nb2 * sizeof(double));
  if (e == hipSuccess && kl && host) e = alloc(dkl, (size_t)E * sizeof(double));
  double *fo = device_output(f, mem_kind, df), *klo = device_output(kl, mem_kind, dkl);
  if (e == hipSuccess) e = phase_enqueue(h, s, (const double*)h->x.get(), (const double*)h->v, acc, feq, nullptr, fo, klo, nullptr, a);
  if (e == hipSuccess) e = device_result(h, f, fo, (size_t)E * nb2 * sizeof(double));
  if (e == hipSuccess) e = device_result(h, kl, klo, (size_t)E * sizeof(double));
  return hip_tail(h, e, true, "pic_phase_kl_smooth");
}

int pic_phase_kl_smooth_vjp(pic_handle* h, const pic_phase_spec* s, const double* cot_kl, int mem_kind, void* g_x, void* g_v) {
  int rc = phase_check(h, s, mem_kind, "pic_phase_kl_smooth_vjp");
  if (rc) return rc;
  if (!s->feq || !cot_kl) return fail(h, PIC_EINVAL, "pic_phase_kl_smooth_vjp: needs spec->feq and cot_kl");
  if (!g_x && !g_v) return PIC_OK;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs;
  const size_t nb2 = (size_t)s->nx * s->nv, pbytes = (size_t)E * h->cfg.N * sizeof(double);
  const size_t feq_bytes = (s->feq_per_env ? E : 1) * nb2 * sizeof(double);
  DeviceBuf<unsigned long long> acc;
  DeviceBuf<double> dfeq, dcot, dg, dgx, dgv;
  const double *feq = nullptr, *cot = nullptr;
  PhaseArgs a;
  const bool host = mem_kind == PIC_HOST;       // host memory goes through device buffers of this call, and so does a null output
  hipError_t e = alloc_zeroed(acc, (size_t)E * nb2 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess && s->feq_mem_kind == PIC_HOST) e = alloc(dfeq, feq_bytes);
  if (e == hipSuccess) e = device_input(h, s->feq, s->feq_mem_kind, feq_bytes, dfeq, &feq);
  if (e == hipSuccess && host) e = alloc(dcot, (size_t)E * sizeof(double));
  if (e == hipSuccess) e = device_input(h, cot_kl, mem_kind, (size_t)E * sizeof(double), dcot, &cot);
  if (e == hipSuccess) e = alloc(dg, (size_t)E * nb2 * sizeof(double));
  if (e == hipSuccess && (host || !g_x)) e = alloc(dgx, pbytes);
  if (e == hipSuccess && (host || !g_v)) e = alloc(dgv, pbytes);
  double* gx = g_x && !host ? static_cast<double*>(g_x) : dgx.get();
  double* gv = g_v && !host ? static_cast<double*>(g_v) : dgv.get();
  if (e == hipSuccess) e = phase_enqueue(h, s, (const double*)h->x.get(), (const double*)h->v, acc, feq, cot, nullptr, nullptr, dg, a);
  if (e == hipSuccess) {
    const double norm = phase_norm(h, s);
    const dim3 grid((unsigned)((h->cfg.N + BLOCK - 1) / BLOCK), (unsigned)E);
    hipLaunchKernelGGL(phase_vjp_kernel, grid, dim3(BLOCK), 0, h->stream, (const double*)h->x.get(), (const double*)h->v,
                       (const double*)dg, a, norm * a.rdx, norm * a.rdv, gx, gv);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = device_result(h, g_x, gx, pbytes);
  if (e == hipSuccess) e = device_result(h, g_v, gv, pbytes);
  return hip_tail(h, e, true, "pic_phase_kl_smooth_vjp");
}

// ---------------------------------------------------------------------------------------------
// Forward mode of the smoothed KL (include/picstep.h: pic_phase_kl_smooth_jvp; pic_phase.h)
// ---------------------------------------------------------------------------------------------
// chunks of kJvpChunkTiles tiles per environment: a constant of N alone
static int phase_jvp_chunks(const pic_handle* h) {
  return (int)(((h->cfg.N + 1) / 2 + kJvpChunkTiles - 1) / kJvpChunkTiles);
}

// a row of n ones in device memory (the unit cotangents the finishing kernel scales g with)
static hipError_t phase_fill_ones(pic_handle* h, double* dst, size_t n) {
  const std::vector<double> ones(n, 1.0);
  hipError_t e = hipMemcpyAsync(dst, ones.data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(h->stream);      // (`ones` goes away behind this call)
}

// The two kernels behind a deposit and finish that left the unit-cotangent grid g of the particles x, v [env][ld]:
// out[d * out_dstride + env] = sum_k dKL~/dx_k dx_k + dKL~/dv_k dv_k for the K directions of `j` (dx, dv, dstride, erow set by
// the caller; part: [K][env][chunks] device memory)
static hipError_t phase_jvp_enqueue(pic_handle* h, const pic_phase_spec* s, const PhaseArgs& a, const double* x, const double* v,
                                    const double* g, PhaseJvpArgs j, int K, double* out, long long out_dstride) {
  const int E = h->cfg.num_envs;
  j.K = K; j.num_envs = E; j.chunks = phase_jvp_chunks(h);
  const double norm = phase_norm(h, s);
  const dim3 grid((unsigned)j.chunks, (unsigned)E);
  if (K == 1) hipLaunchKernelGGL(phase_jvp_kernel<1>, grid, dim3(BLOCK), 0, h->stream, x, v, g, a, norm * a.rdx, norm * a.rdv, j);
  else if (K <= 4) hipLaunchKernelGGL(phase_jvp_kernel<4>, grid, dim3(BLOCK), 0, h->stream, x, v, g, a, norm * a.rdx, norm * a.rdv, j);
  else hipLaunchKernelGGL(phase_jvp_kernel<8>, grid, dim3(BLOCK), 0, h->stream, x, v, g, a, norm * a.rdx, norm * a.rdv, j);
  hipLaunchKernelGGL(phase_jvp_finish_kernel, dim3(E, K), dim3(1), 0, h->stream, (const double*)j.part, j.chunks, E, out, out_dstride);
  return hipGetLastError();
}

int pic_phase_kl_smooth_jvp(pic_handle* h, const pic_phase_spec* s, int K, const void* d_x, const void* d_v, int mem_kind,
                            double* d_kl) {
  int rc = phase_check(h, s, mem_kind, "pic_phase_kl_smooth_jvp");
  if (rc) return rc;
  if (!s->feq || !d_kl) return fail(h, PIC_EINVAL, "pic_phase_kl_smooth_jvp: needs spec->feq and d_kl");
  if (K < 1 || K > kMaxTangents) return fail(h, PIC_EINVAL, "pic_phase_kl_smooth_jvp: need 1 <= K <= " + std::to_string(kMaxTangents));
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int E = h->cfg.num_envs, chunks = phase_jvp_chunks(h);
  const size_t nb2 = (size_t)s->nx * s->nv, N = h->cfg.N, pbytes = (size_t)K * E * N * sizeof(double);
  const size_t feq_bytes = (s->feq_per_env ? E : 1) * nb2 * sizeof(double), obytes = (size_t)K * E * sizeof(double);
  DeviceBuf<unsigned long long> acc;
  DeviceBuf<double> dfeq, dones, dg, dpart, ddx, ddv, dout;
  const double *feq = nullptr, *tx = nullptr, *tv = nullptr;
  PhaseArgs a;
  const bool host = mem_kind == PIC_HOST;       // host memory goes through device buffers of this call
  hipError_t e = alloc_zeroed(acc, (size_t)E * nb2 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess && s->feq_mem_kind == PIC_HOST) e = alloc(dfeq, feq_bytes);
  if (e == hipSuccess) e = device_input(h, s->feq, s->feq_mem_kind, feq_bytes, dfeq, &feq);
  if (e == hipSuccess) e = alloc(dones, (size_t)E * sizeof(double));
  if (e == hipSuccess) e = phase_fill_ones(h, dones, (size_t)E);
  if (e == hipSuccess) e = alloc(dg, (size_t)E * nb2 * sizeof(double));
  if (e == hipSuccess) e = alloc(dpart, (size_t)K * E * chunks * sizeof(double));
  if (e == hipSuccess && host && d_x) e = alloc(ddx, pbytes);
  if (e == hipSuccess && host && d_v) e = alloc(ddv, pbytes);
  if (e == hipSuccess) e = device_input(h, static_cast<const double*>(d_x), mem_kind, pbytes, ddx, &tx);
  if (e == hipSuccess) e = device_input(h, static_cast<const double*>(d_v), mem_kind, pbytes, ddv, &tv);
  if (e == hipSuccess && host) e = alloc(dout, obytes);
  double* out = device_output(d_kl, mem_kind, dout);
  const double *x = (const double*)h->x.get(), *v = (const double*)h->v;
  if (e == hipSuccess) e = phase_enqueue(h, s, x, v, acc, feq, dones, nullptr, nullptr, dg, a);
  if (e == hipSuccess) {
    PhaseJvpArgs j{};
    j.dx = tx; j.dv = tv; j.dstride = (long long)((size_t)E * N); j.erow = (long long)N; j.part = dpart;
    e = phase_jvp_enqueue(h, s, a, x, v, dg, j, K, out, (long long)E);
  }
  if (e == hipSuccess) e = device_result(h, d_kl, out, obytes);
  return hip_tail(h, e, true, "pic_phase_kl_smooth_jvp");
}
