// pic_pool_ln.h -- pooled particle features with a LayerNorm inside the per-particle layer (include/picstep.h: pic_pool_ln,
// pic_pool_ln_vjp; pic_pool_ln_jvp: 7t): per environment
//   out_k = (1/N) sum_i act(gamma_k y_ik + beta_k),   y_ik = (z_ik - mu_i) r_i,   r_i = 1 / sqrt(var_i + eps)
// with pic_pool's z_ik and mu_i, var_i the mean and the biased variance of z_i. over the H units.  The passes are pic_pool.h's
// skeleton with the layer type PoolLn: this file holds only what is the LayerNorm's.  z is three multiply-adds and is recomputed
// in every walk, so nothing of size [H] is kept per particle.  New are the walks before the terms: sum z, then sum d^2 (forward,
// and the VJP's max pass: r_max), in the VJP one more for m1 and m2, in the JVP two more for dmu and p.  -ffp-contract=off.
#pragma once
#include "pic_pool.h"

namespace {

constexpr double kLnFwdUp = 0x1.0000000000004p+0;      // 1 + 2^-50: above the rounding of B_k and of n_ik
constexpr double kLnVjpUp = 0x1.0000000001p+0;         // 1 + 2^-40: above the rounding of the VJP's bounds and terms
constexpr double kLnOverflow = 0x1p+500;               // a bound of |z| above this: the environment is NaN

struct PoolLnArgs {
  unsigned long long* rmax;    // [env] bit pattern of max r (VJP, JVP; zero between calls), or null
  double eps, Hd, sqrtH;       // Hd = (double)H, sqrtH = sqrt(Hd)
};

// The parameters of unit k: W_k. and b_k, gamma_k, beta_k (P = 6H: W [H][3], b [H], gamma [H], beta [H])
struct LnRow { double w0, w1, w2, b, g, be; };

__device__ __forceinline__ LnRow ln_row(const double* __restrict__ p, int H, int k) {
  return LnRow{p[3 * k], p[3 * k + 1], p[3 * k + 2], p[3 * H + k], p[4 * H + k], p[5 * H + k]};
}

// Whether the environment is NaN as a whole: a non-finite W_k. or b_k (the mean over k spreads it), or z or var that could
// overflow, max_k ((|W_k0| + |W_k1|) + |W_k2| u_max) + |b_k| > 2^500; with a cotangent (VJP) a non-finite gamma_k, beta_k or
// cot_k too.  The same value in every thread of the workgroup (a barrier).
__device__ __forceinline__ bool ln_env_bad(const double* __restrict__ p, const double* __restrict__ cot, int H, double umx) {
  int bad = 0;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    const LnRow w = ln_row(p, H, k);
    const double B = ((fabs(w.w0) + fabs(w.w1)) + fabs(w.w2) * umx) + fabs(w.b);
    if (!(B <= kLnOverflow)) bad = 1;                                   // (a NaN or an infinity among them too)
    if (cot && !(pool_finite(w.g) && pool_finite(w.be) && pool_finite(cot[k]))) bad = 1;
  }
  return __syncthreads_or(bad) != 0;
}

// mu_i and r_i of a lane's particles: two walks over k
__device__ __forceinline__ void ln_stats(const double* __restrict__ p, int H, const PoolLnArgs& n, const PoolLane& q,
                                         double (&mu)[kPoolPerLane], double (&r)[kPoolPerLane]) {
  double acc[kPoolPerLane];
#pragma unroll
  for (int j = 0; j < kPoolPerLane; ++j) acc[j] = 0.0;
  for (int k = 0; k < H; ++k) {
    const double w0 = p[3 * k], w1 = p[3 * k + 1], w2 = p[3 * k + 2], bk = p[3 * H + k];
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) acc[j] = acc[j] + pool_pre(w0, w1, w2, bk, q.c[j], q.s[j], q.u[j]);
  }
#pragma unroll
  for (int j = 0; j < kPoolPerLane; ++j) {
    mu[j] = acc[j] / n.Hd;
    acc[j] = 0.0;
  }
  for (int k = 0; k < H; ++k) {
    const double w0 = p[3 * k], w1 = p[3 * k + 1], w2 = p[3 * k + 2], bk = p[3 * H + k];
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) {
      const double d = pool_pre(w0, w1, w2, bk, q.c[j], q.s[j], q.u[j]) - mu[j];
      acc[j] = acc[j] + d * d;
    }
  }
#pragma unroll
  for (int j = 0; j < kPoolPerLane; ++j) r[j] = 1.0 / sqrt(acc[j] / n.Hd + n.eps);
}

// n_ik = gamma_k y_ik + beta_k (the product rounded first) and y_ik
__device__ __forceinline__ double ln_norm(const LnRow& w, double c, double s, double u, double mu, double r, double& y) {
  const double d = pool_pre(w.w0, w.w1, w.w2, w.b, c, s, u) - mu;
  y = d * r;
  const double gy = w.g * y;
  return gy + w.be;
}

// the unit word of out_k: tanh is bounded by 1 = 2^0; relu by B_k = |gamma_k| sqrt(H) + |beta_k|, rounded up (|y_ik| < sqrt(H))
__device__ __forceinline__ int ln_fwd_unit(const LnRow& w, int activation, double sqrtH, int bitsN) {
  if (!(pool_finite(w.g) && pool_finite(w.be))) return kPoolNan;
  if (activation == PIC_ACT_TANH) return bitsN - 61;
  return pool_unit((fabs(w.g) * sqrtH + fabs(w.be)) * kLnFwdUp, bitsN);
}

// the units of the six parameter sums of unit k, given D_max = max_k |cot_k| |gamma_k| / N
struct LnVjpUnits { int w, g, b; };

__device__ __forceinline__ LnVjpUnits ln_vjp_units(double gamma, double cot, double dmax, double rmx, double umx, double Nd,
                                                   double sqrtH, int bitsN) {
  const double ck = fabs(cot) / Nd, dk = (fabs(cot) * fabs(gamma)) / Nd;
  const double bw = (((dk + (1.0 + sqrtH) * dmax) * rmx) * (umx > 1.0 ? umx : 1.0)) * kLnVjpUp;
  return LnVjpUnits{pool_unit(bw, bitsN), pool_unit((ck * sqrtH) * kLnVjpUp, bitsN), pool_unit(ck * kLnVjpUp, bitsN)};
}

// D_max of the environment through an LDS word: the same value in every thread of the workgroup (two barriers)
__device__ __forceinline__ double ln_dmax(const double* __restrict__ p, const double* __restrict__ cot, int H, double Nd) {
  __shared__ unsigned long long word;
  if (threadIdx.x == 0) word = 0ull;
  __syncthreads();
  unsigned long long m = 0ull;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) mom_max_bits(m, (fabs(cot[k]) * fabs(p[4 * H + k])) / Nd);
  if (m) atomicMax(&word, m);
  __syncthreads();
  return __longlong_as_double((long long)word);
}

// Z_max = max_k Z_k of a (direction, environment) through an LDS word (tp: the direction's tangent parameters, null = 0); a Z_k
// that is not finite saturates it.  The same value in every thread of the workgroup (three barriers).
__device__ __forceinline__ double ln_jvp_zmax(const double* __restrict__ p, const double* __restrict__ tp, int H, const PoolJvpMax& mx) {
  __shared__ unsigned long long word;
  if (threadIdx.x == 0) word = 0ull;
  __syncthreads();
  unsigned long long m = 0ull;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    const LnRow d = tp ? ln_row(tp, H, k) : LnRow{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    mom_max_bits(m, pool_jvp_z(p[3 * k], p[3 * k + 1], p[3 * k + 2], d, mx));
  }
  if (m) atomicMax(&word, m);
  __syncthreads();
  const double zmax = __longlong_as_double((long long)word);
  __syncthreads();                                         // (the next direction's call clears the word)
  return zmax;
}

// The LayerNorm's layer type for pic_pool.h's skeleton (what a layer supplies: there).  The VJP has six sums per unit (g_W_k*
// and g_b_k in one unit word, g_gamma_k and g_beta_k in one each) and walks k once more before the skeleton's walk.
struct PoolLn {
  static constexpr int kSums = 6, kUnits = 3;
  using Row = LnRow;
  struct Stats { double mu[kPoolPerLane], r[kPoolPerLane], m1[kPoolPerLane], m2[kPoolPerLane]; };      // (m1, m2: the VJP's)
  const double* __restrict__ p;
  PoolLnArgs n;
  int H, activation, bitsN;
  double rmx = 0.0, dmax = 0.0;      // the environment's largest r_i and D_max (vjp_env)

  __device__ __forceinline__ PoolLn(const PoolArgs& a, const PoolLnArgs& n_, int env)
      : p(a.params + (size_t)env * a.env_params), n(n_), H(a.H), activation(a.activation), bitsN(a.bitsN) {}
  __device__ __forceinline__ Row row(int k) const { return ln_row(p, H, k); }
  __device__ __forceinline__ bool env_bad(const double* cot, double umx) const { return ln_env_bad(p, cot, H, umx); }
  __device__ __forceinline__ void prepare(const PoolLane& q, Stats& st) const { ln_stats(p, H, n, q, st.mu, st.r); }
  __device__ __forceinline__ double arg(const Row& w, const PoolLane& q, const Stats& st, int j, double& y) const {
    return ln_norm(w, q.c[j], q.s[j], q.u[j], st.mu[j], st.r[j], y);
  }
  __device__ __forceinline__ int fwd_unit(int k, double) const { return ln_fwd_unit(row(k), activation, n.sqrtH, bitsN); }
  __device__ __forceinline__ void vjp_env(const double* ge, double Nd, int env) {
    rmx = __longlong_as_double((long long)n.rmax[env]);
    dmax = ln_dmax(p, ge, H, Nd);
  }
  __device__ __forceinline__ LnVjpUnits units(int k, double gk, double umx, double Nd) const {
    return ln_vjp_units(p[4 * H + k], gk, dmax, rmx, umx, Nd, n.sqrtH, bitsN);
  }
  __device__ __forceinline__ int vjp_unit(int m, int k, double gk, double umx, double Nd) const {
    const LnVjpUnits us = units(k, gk, umx, Nd);
    return m < 4 ? us.w : (m == 4 ? us.g : us.b);
  }
  __device__ __forceinline__ void vjp_units(int* unit, int k, double gk, double umx, double Nd, bool dep) const {
    const LnVjpUnits ue = units(k, gk, umx, Nd);
    unit[k] = dep ? ue.w : kPoolSkip;
    unit[H + k] = dep ? ue.g : kPoolSkip;
    unit[2 * H + k] = dep ? ue.b : kPoolSkip;
  }
  // the walk over k behind mu and r: m1_i and m2_i, and the deposits of g_gamma, g_beta
  __device__ __forceinline__ void first_walk(const PoolLane& q, Stats& st, const double* __restrict__ ge, double Nd, bool is_tanh,
                                             const int* unit, unsigned long long* sums) const {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) st.m1[j] = st.m2[j] = 0.0;
    for (int k = 0; k < H; ++k) {
      const int ug = unit[H + k], ub = unit[2 * H + k];
      const bool ong = pool_on(ug), onb = pool_on(ub);     // (uniform)
      const LnRow w = ln_row(p, H, k);
      const double ck = ge[k];
      long long pg = 0, pb = 0;
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double nn = ln_norm(w, q.c[j], q.s[j], q.u[j], st.mu[j], st.r[j], y);
        const double dn = pool_dn(nn, ck, Nd, is_tanh), dy = dn * w.g;
        st.m1[j] = st.m1[j] + dy;
        st.m2[j] = st.m2[j] + dy * y;
        if (ong && q.on[j]) pg += __double2ll_rn(ldexp(dn * y, -ug));
        if (onb && q.on[j]) pb += __double2ll_rn(ldexp(dn, -ub));
      }
      if (ong) {
        pg = wave_sum_i64(pg);
        if (lane == 0 && pg) atomicAdd(sums + 4 * H + k, (unsigned long long)pg);
      }
      if (onb) {
        pb = wave_sum_i64(pb);
        if (lane == 0 && pb) atomicAdd(sums + 5 * H + k, (unsigned long long)pb);
      }
    }
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) {
      st.m1[j] = st.m1[j] / n.Hd;
      st.m2[j] = st.m2[j] / n.Hd;
    }
  }
  // dz_ik from dn_ik = (cot_k a_ik) / N
  __device__ __forceinline__ double back(const Row& w, double dn, double y, const Stats& st, int j) const {
    const double dy = dn * w.g;
    return ((dy - st.m1[j]) - y * st.m2[j]) * st.r[j];
  }
  __device__ __forceinline__ void clear(int env) const { n.rmax[env] = 0ull; }

  // forward mode (pic_pool_ln_jvp): the tangent row of unit k, Z_max and r_max of a (direction, environment), the unit word of
  // d_out_k, the two walks over k for dmu_i and p_i of every direction of a group, and dn from dz
  static constexpr bool kRmax = true;
  template <int KD> struct Tan { double dmu[KD][kPoolPerLane], p[KD][kPoolPerLane]; };
  __device__ __forceinline__ static Row trow(const double* __restrict__ tp, int H, int k) {
    return tp ? ln_row(tp, H, k) : LnRow{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  }
  __device__ __forceinline__ PoolJvpEnv jvp_env(const double* __restrict__ tp, const PoolJvpMax& m, int env) const {
    return PoolJvpEnv{m, ln_jvp_zmax(p, tp, H, m), __longlong_as_double((long long)n.rmax[env])};
  }
  // |dgamma_k| sqrt(H) + |gamma_k| (Z_k + (1 + sqrt(H)) Z_max) r_max + |dbeta_k|, rounded up
  __device__ __forceinline__ int jvp_unit(int k, const double* __restrict__ tp, const PoolJvpEnv& e) const {
    const Row w = row(k), d = trow(tp, H, k);
    if (!(pool_finite(w.g) && pool_finite(w.be) && pool_finite(d.g) && pool_finite(d.be))) return kPoolNan;
    const double Zk = pool_jvp_z(w.w0, w.w1, w.w2, d, e.m);
    const double bz = (Zk + (1.0 + n.sqrtH) * e.zmax) * e.rmx;
    return pool_unit(((fabs(d.g) * n.sqrtH + fabs(w.g) * bz) + fabs(d.be)) * kPoolJvpUp, bitsN);
  }
  template <int KD>
  __device__ __forceinline__ void jvp_walks(const PoolLane& q, const Stats& st, const PoolTan<KD>& tn, const double* const (&tp)[KD],
                                            const bool (&live)[KD], Tan<KD>& lt) const {
    double acc[KD][kPoolPerLane];
#pragma unroll
    for (int d = 0; d < KD; ++d)
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) acc[d][j] = 0.0;
    for (int k = 0; k < H; ++k) {
      const Row w = row(k);
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (!live[d]) continue;                            // (uniform)
        const Row tw = trow(tp[d], H, k);
#pragma unroll
        for (int j = 0; j < kPoolPerLane; ++j)
          acc[d][j] = acc[d][j] + pool_dz(w.w0, w.w1, w.w2, tw, q.c[j], q.s[j], q.u[j], tn.tq[d][j], tn.tu[d][j]);
      }
    }
#pragma unroll
    for (int d = 0; d < KD; ++d)
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        lt.dmu[d][j] = acc[d][j] / n.Hd;
        acc[d][j] = 0.0;
      }
    for (int k = 0; k < H; ++k) {
      const Row w = row(k);
      double y[kPoolPerLane];
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) y[j] = (pool_pre(w.w0, w.w1, w.w2, w.b, q.c[j], q.s[j], q.u[j]) - st.mu[j]) * st.r[j];
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (!live[d]) continue;
        const Row tw = trow(tp[d], H, k);
#pragma unroll
        for (int j = 0; j < kPoolPerLane; ++j) {
          const double e = pool_dz(w.w0, w.w1, w.w2, tw, q.c[j], q.s[j], q.u[j], tn.tq[d][j], tn.tu[d][j]) - lt.dmu[d][j];
          acc[d][j] = acc[d][j] + y[j] * e;
        }
      }
    }
#pragma unroll
    for (int d = 0; d < KD; ++d)
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) lt.p[d][j] = acc[d][j] / n.Hd;
  }
  // dn_ik = (dgamma_k y_ik + gamma_k dy_ik) + dbeta_k,   dy_ik = (e_ik - y_ik p_i) r_i,   e_ik = dz_ik - dmu_i
  template <int KD>
  __device__ __forceinline__ double jvp_dn(const Row& w, const Row& tw, double dz, double y, const Stats& st, const Tan<KD>& lt, int d,
                                           int j) const {
    const double e = dz - lt.dmu[d][j];
    const double dy = (e - y * lt.p[d][j]) * st.r[j];
    const double gy = tw.g * y, gd = w.g * dy;
    return (gy + gd) + tw.be;
  }
};

// The VJP's max pass: pool_max_kernel's word (max |u|, saturated by a non-finite u or q) and next to it the environment's largest
// r_i in rmax[env].  It walks k twice per particle.  Grid: the passes'.
__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_max_kernel(PoolArgs a, PoolLnArgs n) {
  const int env = blockIdx.y, H = a.H;
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  long long t0, t1;
  pool_range(a, t0, t1);
  unsigned long long mb = 0ull, rb = 0ull;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    PoolLane q;
    pool_load(a, xe, ve, tc, t1, q);
    double mu[kPoolPerLane], r[kPoolPerLane];
    ln_stats(p, H, n, q, mu, r);
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) {
      if (!q.on[j]) continue;
      mom_max_bits(mb, fabs(q.u[j]));
      if (!pool_finite(q.c[j])) mb = kMomInfBits;          // (cos of a non-finite q is NaN)
      mom_max_bits(rb, r[j]);
    }
  }
  block_max_to(__longlong_as_double((long long)mb), a.umax + env);
  block_max_to(__longlong_as_double((long long)rb), n.rmax + env);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_kernel(PoolArgs a, PoolLnArgs n) { pool_fwd_body(a, PoolLn(a, n, blockIdx.y)); }

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_finish_kernel(PoolArgs a, PoolLnArgs n, double* __restrict__ out) {
  pool_finish_body(a, PoolLn(a, n, blockIdx.x), out);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_vjp_kernel(PoolArgs a, PoolLnArgs n, PoolVjpArgs g) {
  PoolLn layer(a, n, blockIdx.y);
  pool_vjp_body(a, g, layer);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_vjp_finish_kernel(PoolArgs a, PoolLnArgs n, PoolVjpArgs g, double* __restrict__ gE) {
  PoolLn layer(a, n, blockIdx.x);
  pool_vjp_finish_body(a, g, layer, gE);
}

// directions of a group of pool_ln_jvp_kernel: with 4 hipcc reports no scratch either, but 30 AGPRs of spills and
// one wave per SIMD, and the call measured 1.4 x slower
constexpr int kPoolLnJvpDirs = 2;

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_jvp_max_kernel(PoolArgs a, PoolLnArgs n, PoolJvpArgs t) {
  pool_jvp_max_body(a, t, PoolLn(a, n, blockIdx.y), n.rmax);
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_jvp_kernel(PoolArgs a, PoolLnArgs n, PoolJvpArgs t) {
  pool_jvp_body<PoolLn, kPoolLnJvpDirs>(a, t, PoolLn(a, n, blockIdx.y));
}

__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_jvp_finish_kernel(PoolArgs a, PoolLnArgs n, PoolJvpArgs t, double* __restrict__ d_out) {
  pool_jvp_finish_body(a, t, PoolLn(a, n, blockIdx.x), d_out);
}

}  // namespace
