// host_pool.h -- included by picstep.hip alone, inside its extern "C" block behind host_diff.h
#pragma once
// ---------------------------------------------------------------------------------------------
// Pooled particle features (include/picstep.h: pic_pool, pic_pool_vjp; pic_pool.h) and the same with a LayerNorm
// inside the per-particle layer (pic_pool_ln, pic_pool_ln_vjp; pic_pool_ln.h): one begin, one forward, one VJP
// and one JVP (pic_pool_jvp, pic_pool_ln_jvp) for both layers; call.shape.ln picks the kernels
// ---------------------------------------------------------------------------------------------
// what is wrong with a spec (null: nothing)
static const char* pool_spec_error(const pic_pool_spec* s) {
  if (!s) return "spec is NULL";
  if (s->hidden < 1 || s->hidden > kPoolMaxHidden) return "hidden must be 1..256";
  if (s->activation != PIC_ACT_TANH && s->activation != PIC_ACT_RELU) return "activation must be PIC_ACT_TANH or PIC_ACT_RELU";
  if (s->per_env != 0 && s->per_env != 1) return "per_env must be 0 or 1";
  if (s->params_mem_kind != PIC_HOST && s->params_mem_kind != PIC_DEVICE) return "bad params_mem_kind";
  if (!s->params) return "params is NULL";
  if (!std::isfinite(s->v_scale)) return "v_scale is not finite";
  return nullptr;
}

// the members a pic_pool_ln_spec shares with a pic_pool_spec
static pic_pool_spec pool_ln_base(const pic_pool_ln_spec* s) {
  return pic_pool_spec{s->hidden, s->activation, s->per_env, s->params_mem_kind, s->v_scale, s->params};
}

// what is wrong with a pic_pool_ln_spec (null: nothing): pic_pool's checks on the shared members, then its own
static const char* pool_ln_spec_error(const pic_pool_ln_spec* s) {
  if (!s) return "spec is NULL";
  const pic_pool_spec base = pool_ln_base(s);
  if (const char* bad = pool_spec_error(&base)) return bad;
  if (!(std::isfinite(s->eps) && s->eps > 0.0)) return "eps must be finite and > 0";
  if (!(std::isfinite(s->period) && s->period >= 0.0)) return "period must be finite and >= 0";
  return nullptr;
}

// whether a call may read the handle's stored particles (x = v = NULL); nothing is enqueued or changed
static int pool_stored_check(pic_handle* h, const char* who) {
  if (h->fmt != FMT_F64)
    return fail(h, PIC_EINVAL, std::string(who) + ": the stored particles need float64 particles with float64 positions (float32 and "
                                                  "fixed32 are not differentiated); pass x and v");
  if (!h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first");
  if (h->sched.mid_stage) return fail(h, PIC_ESTATE, std::string(who) + ": a staged step is in progress");
  return PIC_OK;
}

// one call: what pool_begin makes of the arguments
struct PoolCall {
  PoolCallShape shape;
  PoolViews w;
  PoolArgs a;
  PoolLnArgs n;              // (shape.ln)
  dim3 grid;
};

// One call's checks, block and kernel arguments.  `result`: out (forward), cot (VJP) or d_out (JVP), which must not be NULL.
// c.shape: vjp, g_*, jvp, K, d_* and ln as the caller set them (ln: the parameters are 6H per vector); the rest is filled in here.
// Everything is refused before anything is enqueued; on PIC_OK the block is carved for c.shape, its sums are zero, the
// parameters and the particles are on the device and c.a, c.grid are the passes'.
static int pool_begin(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, const void* result, const char* result_name,
                      int mem_kind, const char* who, PoolCall& c) {
  if (!h) return PIC_EINVAL;
  if (int rc = check_mem_kind(h, mem_kind, who)) return rc;
  if (const char* bad = pool_spec_error(s)) return fail(h, PIC_EINVAL, std::string(who) + ": " + bad);
  if (!result) return fail(h, PIC_EINVAL, std::string(who) + ": " + result_name + " is NULL");
  if (c.shape.jvp && (c.shape.K < 1 || c.shape.K > kMaxTangents))
    return fail(h, PIC_EINVAL, std::string(who) + ": need 1 <= K <= " + std::to_string(kMaxTangents));
  if (!x != !v) return fail(h, PIC_EINVAL, std::string(who) + ": x and v must both be given or both be NULL");
  if (!x)
    if (int rc = pool_stored_check(h, who)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  PoolCallShape& shape = c.shape; PoolViews& w = c.w; PoolArgs& a = c.a;
  const size_t E = h->cfg.num_envs, N = h->cfg.N, H = (size_t)s->hidden, P = (shape.ln ? 6 : 4) * H;
  shape.H = H; shape.N = N; shape.per_env = s->per_env != 0;
  shape.host = mem_kind == PIC_HOST; shape.params_host = s->params_mem_kind == PIC_HOST; shape.xv = x != nullptr;
  const size_t cap_before = h->pool_cap;      // (the block grows only: another capacity is another allocation)
  if (int rc = call_reserve(h, h->pool_block, &h->pool_cap, who, "the working memory", w,
                            [&](Carver cv, PoolViews& k) { return pool_parts(cv, block_dims(h), shape, k); }))
    return rc;
  const size_t accn = E * (shape.vjp ? P : (shape.jvp ? (size_t)shape.K : 1) * H), zero = (size_t)((char*)(w.acc + accn) - (char*)w.max);
  if (h->pool_cap != cap_before || zero > h->pool_zero) {
    h->pool_zero = 0;
    HIPCHK(h, hipMemsetAsync(w.max, 0, Carver::upto(w.max, w.acc + accn), h->stream));
  }
  h->pool_zero = zero;       // (what lies behind may hold this call's copies)
  a = PoolArgs{};
  const double* params = nullptr;
  HIPCHK(h, device_input(h, s->params, s->params_mem_kind, (shape.per_env ? E : 1) * P * sizeof(double), w.params, &params));
  a.params = params;
  a.env_params = shape.per_env ? (long long)P : 0;
  if (x) {
    HIPCHK(h, device_input(h, static_cast<const double*>(x), mem_kind, E * N * sizeof(double), w.x, &a.x));
    HIPCHK(h, device_input(h, static_cast<const double*>(v), mem_kind, E * N * sizeof(double), w.v, &a.v));
    a.ld = (long long)N;
  } else {
    a.x = static_cast<const double*>(h->x.get());
    a.v = static_cast<const double*>(h->v);
    a.ld = h->ld;
  }
  a.umax = w.max; a.acc = w.acc;
  a.N = (long long)N; a.L = h->cfg.L; a.v_scale = s->v_scale; a.H = (int)H; a.activation = s->activation;
  while (((int64_t)1 << a.bitsN) < (int64_t)N) ++a.bitsN;
  static_assert(kPoolChunkTiles == (long long)POOL_BLOCK * kPoolTiles, "pool_plan's chunk is the kernels'");
  const PoolPlan plan = pool_plan(E, N);
  a.chunks_per_wg = plan.chunks_per_wg;
  c.grid = dim3((unsigned)plan.workgroups, (unsigned)E);
  return PIC_OK;
}

// pool_begin for a pic_pool_ln_spec: its own checks, then pic_pool's with the shared members; c.n are the LayerNorm's arguments
static int pool_ln_begin(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, const void* result,
                         const char* result_name, int mem_kind, const char* who, PoolCall& c) {
  if (!h) return PIC_EINVAL;
  if (const char* bad = pool_ln_spec_error(s)) return fail(h, PIC_EINVAL, std::string(who) + ": " + bad);
  const pic_pool_spec base = pool_ln_base(s);
  c.shape.ln = true;
  if (int rc = pool_begin(h, &base, x, v, result, result_name, mem_kind, who, c)) return rc;
  if (s->period > 0.0) c.a.L = s->period;
  c.n = PoolLnArgs{};
  c.n.rmax = c.shape.vjp || c.shape.jvp ? c.w.max + h->cfg.num_envs : nullptr;
  c.n.eps = s->eps; c.n.Hd = (double)c.a.H; c.n.sqrtH = std::sqrt(c.n.Hd);
  return PIC_OK;
}

// the tail of a pool call: a failed call leaves the sums unknown
static int pool_end(pic_handle* h, hipError_t e, bool wait, const char* who) {
  const int rc = hip_tail(h, e, wait, who);
  if (rc) h->pool_zero = 0;
  return rc;
}

// the forward of a call that has begun: the max pass (u_max and the non-finite mark alone, for both layers), the pass, the finish
static int pool_forward(pic_handle* h, const PoolCall& c, int mem_kind, double* out, const char* who) {
  const PoolArgs& a = c.a;
  const dim3 block(POOL_BLOCK), envs(h->cfg.num_envs);
  double* dev = device_output(out, mem_kind, c.w.out);
  hipLaunchKernelGGL(pool_max_kernel, c.grid, block, 0, h->stream, a);
  if (c.shape.ln) {
    hipLaunchKernelGGL(pool_ln_kernel, c.grid, block, 0, h->stream, a, c.n);
    hipLaunchKernelGGL(pool_ln_finish_kernel, envs, block, 0, h->stream, a, c.n, dev);
  } else {
    hipLaunchKernelGGL(pool_kernel, c.grid, block, 0, h->stream, a);
    hipLaunchKernelGGL(pool_finish_kernel, envs, block, 0, h->stream, a, dev);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = device_result(h, out, dev, (size_t)h->cfg.num_envs * a.H * sizeof(double));
  return pool_end(h, e, mem_kind == PIC_HOST, who);        // device outputs stay stream-ordered
}

// the shape of a VJP call that wants these outputs
static PoolCallShape pool_vjp_shape(const void* g_x, const void* g_v, const double* g_params) {
  PoolCallShape shape;
  shape.vjp = true; shape.g_x = g_x != nullptr; shape.g_v = g_v != nullptr; shape.g_params = g_params != nullptr;
  return shape;
}

// the VJP of a call that has begun: the max pass (the LayerNorm's with r_max), the pass, the finish, the shared parameters' sum
static int pool_backward(pic_handle* h, const PoolCall& c, const double* cot, int mem_kind, void* g_x, void* g_v, double* g_params,
                         const char* who) {
  if (!g_x && !g_v && !g_params) return PIC_OK;
  const PoolArgs& a = c.a;
  const PoolViews& w = c.w;
  const size_t E = h->cfg.num_envs, N = h->cfg.N, P = (c.shape.ln ? 6 : 4) * (size_t)a.H;
  const dim3 block(POOL_BLOCK), envs((unsigned)E);
  PoolVjpArgs g{};
  HIPCHK(h, device_input(h, cot, mem_kind, E * a.H * sizeof(double), w.cot, &g.cot));
  g.g_x = device_output(g_x, mem_kind, w.g_x);
  g.g_v = device_output(g_v, mem_kind, w.g_v);
  g.want_params = g_params != nullptr;
  // the per-environment sums go to the block (shared parameters, or host memory) or straight to the caller
  double* gE = w.gE ? w.gE : g_params;
  double* gp = c.shape.per_env ? gE : device_output(g_params, mem_kind, w.g);
  if (c.shape.ln) {
    hipLaunchKernelGGL(pool_ln_max_kernel, c.grid, block, 0, h->stream, a, c.n);
    hipLaunchKernelGGL(pool_ln_vjp_kernel, c.grid, block, 0, h->stream, a, c.n, g);
    hipLaunchKernelGGL(pool_ln_vjp_finish_kernel, envs, block, 0, h->stream, a, c.n, g, gE);
  } else {
    hipLaunchKernelGGL(pool_max_kernel, c.grid, block, 0, h->stream, a);
    hipLaunchKernelGGL(pool_vjp_kernel, c.grid, block, 0, h->stream, a, g);
    hipLaunchKernelGGL(pool_vjp_finish_kernel, envs, block, 0, h->stream, a, g, gE);
  }
  if (g_params && !c.shape.per_env)
    hipLaunchKernelGGL(policy_grad_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, (const double*)gE, gp,
                       (long long)P, (int)E);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = device_result(h, g_x, g.g_x, E * N * sizeof(double));
  if (e == hipSuccess) e = device_result(h, g_v, g.g_v, E * N * sizeof(double));
  if (e == hipSuccess) e = device_result(h, g_params, gp, (c.shape.per_env ? E : 1) * P * sizeof(double));
  return pool_end(h, e, mem_kind == PIC_HOST, who);
}

// the shape of a JVP call of K directions with these tangents
static PoolCallShape pool_jvp_shape(int K, const void* d_x, const void* d_v, const double* d_params) {
  PoolCallShape shape;
  shape.jvp = true; shape.K = K; shape.d_x = d_x != nullptr; shape.d_v = d_v != nullptr; shape.d_params = d_params != nullptr;
  return shape;
}

// the JVP of a call that has begun, for both layers: the max pass (u_max, the LayerNorm's r_max, every direction's tq_max and
// tu_max), the pass over groups of directions, the finish
static int pool_tangent(pic_handle* h, const PoolCall& c, int params_mem_kind, const void* d_x, const void* d_v, const double* d_params,
                        int mem_kind, double* d_out, const char* who) {
  const PoolArgs& a = c.a;
  const PoolViews& w = c.w;
  const size_t E = h->cfg.num_envs, N = h->cfg.N, K = (size_t)c.shape.K, P = (c.shape.ln ? 6 : 4) * (size_t)a.H;
  const dim3 block(POOL_BLOCK), envs((unsigned)E);
  PoolJvpArgs t{};
  HIPCHK(h, device_input(h, static_cast<const double*>(d_x), mem_kind, K * E * N * sizeof(double), w.d_x, &t.d_x));
  HIPCHK(h, device_input(h, static_cast<const double*>(d_v), mem_kind, K * E * N * sizeof(double), w.d_v, &t.d_v));
  t.dir_params = (long long)((c.shape.per_env ? E : 1) * P);
  HIPCHK(h, device_input(h, d_params, params_mem_kind, K * (size_t)t.dir_params * sizeof(double), w.d_params, &t.d_params));
  t.tmax = w.tmax; t.K = (int)K; t.num_envs = (int)E;
  double* dev = device_output(d_out, mem_kind, w.out);
  static_assert(kPoolMaxDirs == kMaxTangents, "the max pass unrolls over every direction a call may have");
  if (c.shape.ln) {
    const dim3 grid(c.grid.x, c.grid.y, (unsigned)((K + kPoolLnJvpDirs - 1) / kPoolLnJvpDirs));
    hipLaunchKernelGGL(pool_ln_jvp_max_kernel, c.grid, block, 0, h->stream, a, c.n, t);
    hipLaunchKernelGGL(pool_ln_jvp_kernel, grid, block, 0, h->stream, a, c.n, t);
    hipLaunchKernelGGL(pool_ln_jvp_finish_kernel, envs, block, 0, h->stream, a, c.n, t, dev);
  } else {
    const dim3 grid(c.grid.x, c.grid.y, (unsigned)((K + kPoolJvpDirs - 1) / kPoolJvpDirs));
    hipLaunchKernelGGL(pool_jvp_max_kernel, c.grid, block, 0, h->stream, a, t);
    hipLaunchKernelGGL(pool_jvp_kernel, grid, block, 0, h->stream, a, t);
    hipLaunchKernelGGL(pool_jvp_finish_kernel, envs, block, 0, h->stream, a, t, dev);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = device_result(h, d_out, dev, K * E * a.H * sizeof(double));
  return pool_end(h, e, mem_kind == PIC_HOST, who);
}

int pic_pool(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, int mem_kind, double* out) {
  PoolCall c;
  if (int rc = pool_begin(h, s, x, v, out, "out", mem_kind, "pic_pool", c)) return rc;
  return pool_forward(h, c, mem_kind, out, "pic_pool");
}

int pic_pool_vjp(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, const double* cot, int mem_kind, void* g_x,
                 void* g_v, double* g_params) {
  PoolCall c;
  c.shape = pool_vjp_shape(g_x, g_v, g_params);
  if (int rc = pool_begin(h, s, x, v, cot, "cot", mem_kind, "pic_pool_vjp", c)) return rc;
  return pool_backward(h, c, cot, mem_kind, g_x, g_v, g_params, "pic_pool_vjp");
}

int pic_pool_ln(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, int mem_kind, double* out) {
  PoolCall c;
  if (int rc = pool_ln_begin(h, s, x, v, out, "out", mem_kind, "pic_pool_ln", c)) return rc;
  return pool_forward(h, c, mem_kind, out, "pic_pool_ln");
}

int pic_pool_ln_vjp(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, const double* cot, int mem_kind,
                    void* g_x, void* g_v, double* g_params) {
  PoolCall c;
  c.shape = pool_vjp_shape(g_x, g_v, g_params);
  if (int rc = pool_ln_begin(h, s, x, v, cot, "cot", mem_kind, "pic_pool_ln_vjp", c)) return rc;
  return pool_backward(h, c, cot, mem_kind, g_x, g_v, g_params, "pic_pool_ln_vjp");
}

int pic_pool_jvp(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, int K, const void* d_x, const void* d_v,
                 const double* d_params, int mem_kind, double* d_out) {
  PoolCall c;
  c.shape = pool_jvp_shape(K, d_x, d_v, d_params);
  if (int rc = pool_begin(h, s, x, v, d_out, "d_out", mem_kind, "pic_pool_jvp", c)) return rc;
  return pool_tangent(h, c, s->params_mem_kind, d_x, d_v, d_params, mem_kind, d_out, "pic_pool_jvp");
}

int pic_pool_ln_jvp(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, int K, const void* d_x, const void* d_v,
                    const double* d_params, int mem_kind, double* d_out) {
  PoolCall c;
  c.shape = pool_jvp_shape(K, d_x, d_v, d_params);
  if (int rc = pool_ln_begin(h, s, x, v, d_out, "d_out", mem_kind, "pic_pool_ln_jvp", c)) return rc;
  return pool_tangent(h, c, s->params_mem_kind, d_x, d_v, d_params, mem_kind, d_out, "pic_pool_ln_jvp");
}
