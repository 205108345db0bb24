// pic_pool_ln.h -- pooled particle features with a LayerNorm inside the per-particle layer (include/picstep.h: pic_pool_ln,
// pic_pool_ln_vjp): per environment
//   out_k = (1/N) sum_i act(gamma_k y_ik + beta_k),   y_ik = (z_ik - mu_i) r_i,   r_i = 1 / sqrt(var_i + eps)
// with pic_pool's z_ik and mu_i, var_i the mean and the biased variance of z_i. over the H units.  The passes are pic_pool.h's: a
// lane holds kPoolPerLane particles (cos, sin, u) in registers and walks the H rows of the parameters, which are wave-uniform
// loads; z is three multiply-adds and is recomputed in every walk, so nothing of size [H] is kept per particle.  New are the
// walks before the terms: sum z, then sum d^2 (forward, and the VJP's max pass: r_max), and in the VJP one more for m1 and m2.
// The sums over particles are pic_pool's 64-bit integer sums in units known before the pass.  -ffp-contract=off.
#pragma once
#include "pic_pool.h"

namespace {

constexpr double kLnFwdUp = 0x1.0000000000004p+0;      // 1 + 2^-50: above the rounding of B_k and of n_ik
constexpr double kLnVjpUp = 0x1.0000000001p+0;         // 1 + 2^-40: above the rounding of the VJP's bounds and terms
constexpr double kLnOverflow = 0x1p+500;               // a bound of |z| above this: the environment is NaN

struct PoolLnArgs {
  unsigned long long* rmax;    // [env] bit pattern of max r (VJP; zero between calls), or null
  const double* cot;           // [env][H] (VJP), or null
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

// Forward pass: pool_kernel's grid and LDS.  Per chunk a lane computes cos, sin, u of its particles once, then mu and r (two
// walks over k), then for every k its kPoolPerLane terms, rounded to integers.
__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_kernel(PoolArgs a, PoolLnArgs n) {
  __shared__ unsigned long long sums[kPoolMaxHidden];
  __shared__ int unit[kPoolMaxHidden];
  const int env = blockIdx.y, H = a.H, lane = threadIdx.x & 63;
  const unsigned long long mb = a.umax[env];
  if (mb >= kMomInfBits) return;                           // (uniform: the finishing kernel writes NaN)
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  if (ln_env_bad(p, nullptr, H, __longlong_as_double((long long)mb))) return;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    sums[k] = 0ull;
    unit[k] = ln_fwd_unit(ln_row(p, H, k), a.activation, n.sqrtH, a.bitsN);
  }
  __syncthreads();
  long long t0, t1;
  pool_range(a, t0, t1);
  const bool is_tanh = a.activation == PIC_ACT_TANH;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    PoolLane q;
    pool_load(a, xe, ve, tc, t1, q);
    double mu[kPoolPerLane], r[kPoolPerLane];
    ln_stats(p, H, n, q, mu, r);
    for (int k = 0; k < H; ++k) {
      const int ue = unit[k];
      if (ue == kPoolSkip || ue == kPoolNan) continue;     // (uniform)
      const LnRow w = ln_row(p, H, k);
      long long part = 0;
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double nn = ln_norm(w, q.c[j], q.s[j], q.u[j], mu[j], r[j], y);
        const double h = is_tanh ? tanh(nn) : (nn > 0.0 ? nn : 0.0);
        if (q.on[j]) part += __double2ll_rn(ldexp(h, -ue));
      }
      part = wave_sum_i64(part);
      if (lane == 0 && part) atomicAdd(sums + k, (unsigned long long)part);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    const unsigned long long s = sums[k];
    if (s) atomicAdd(a.acc + (size_t)env * H + k, s);
  }
}

// One workgroup per environment: pool_finish_kernel with the LayerNorm's units and NaN rule.
__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_finish_kernel(PoolArgs a, PoolLnArgs n, double* __restrict__ out) {
  const int env = blockIdx.x, H = a.H;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const bool bad = ln_env_bad(p, nullptr, H, finite ? __longlong_as_double((long long)mb) : 0.0) || !finite;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
    unsigned long long* s = a.acc + (size_t)env * H + k;
    const int ue = bad ? kPoolNan : ln_fwd_unit(ln_row(p, H, k), a.activation, n.sqrtH, a.bitsN);
    double r = 0.0;
    if (ue == kPoolNan) r = nan;
    else if (ue != kPoolSkip) r = ldexp((double)(long long)*s, ue) / (double)a.N;
    out[(size_t)env * H + k] = r;
    *s = 0ull;
  }
  __syncthreads();                                         // (every lane has read the max word)
  if (threadIdx.x == 0) a.umax[env] = 0ull;
}

// ---------------------------------------------------------------------------------------------
// The vector-Jacobian product for a cotangent cot [env][H] (pic_pool_ln_vjp)
// ---------------------------------------------------------------------------------------------
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

// the units of the six parameter sums of unit k, given D_max = max_k |cot_k| |gamma_k| / N
struct LnVjpUnits { int w, g, b; };

__device__ __forceinline__ LnVjpUnits ln_vjp_units(double gamma, double cot, double dmax, double rmx, double umx, double Nd,
                                                   double sqrtH, int bitsN) {
  const double ck = fabs(cot) / Nd, dk = (fabs(cot) * fabs(gamma)) / Nd;
  const double bw = (((dk + (1.0 + sqrtH) * dmax) * rmx) * (umx > 1.0 ? umx : 1.0)) * kLnVjpUp;
  return LnVjpUnits{pool_unit(bw, bitsN), pool_unit((ck * sqrtH) * kLnVjpUp, bitsN), pool_unit(ck * kLnVjpUp, bitsN)};
}

// D_max of the environment through an LDS word: the same value in every thread of the workgroup (two barriers)
__device__ __forceinline__ double ln_dmax(const double* __restrict__ p, const double* __restrict__ cot, int H, double Nd,
                                          unsigned long long* word) {
  if (threadIdx.x == 0) *word = 0ull;
  __syncthreads();
  unsigned long long m = 0ull;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) mom_max_bits(m, (fabs(cot[k]) * fabs(p[4 * H + k])) / Nd);
  if (m) atomicMax(word, m);
  __syncthreads();
  return __longlong_as_double((long long)*word);
}

// a_ik and dn_ik = (cot_k a_ik) / N of one term
__device__ __forceinline__ double ln_dn(double nn, double cot, double Nd, bool is_tanh) {
  double act;
  if (is_tanh) {
    const double h = tanh(nn);
    act = 1.0 - h * h;
  } else {
    act = nn > 0.0 ? 1.0 : 0.0;
  }
  return (cot * act) / Nd;
}

// The forward's pass with the activations recomputed, twice: the first walk over k behind mu and r gives m1_i, m2_i and deposits
// g_gamma, g_beta; the second forms dz_ik, sums g_x_i and g_v_i in float64 over ascending k (one thread owns a particle) and
// deposits g_W, g_b.  LDS: 6H sums and 3H unit words.
__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_vjp_kernel(PoolArgs a, PoolLnArgs n, PoolVjpArgs g) {
  __shared__ unsigned long long sums[6 * kPoolMaxHidden];
  __shared__ int unit[3 * kPoolMaxHidden];
  __shared__ unsigned long long dword;
  const int env = blockIdx.y, H = a.H, lane = threadIdx.x & 63;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const double* __restrict__ xe = a.x + (size_t)env * a.ld;
  const double* __restrict__ ve = a.v + (size_t)env * a.ld;
  const double* __restrict__ ge = n.cot + (size_t)env * H;
  const double umx = finite ? __longlong_as_double((long long)mb) : 0.0, Nd = (double)a.N;
  const double rmx = __longlong_as_double((long long)n.rmax[env]);
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const bool bad = ln_env_bad(p, ge, H, umx) || !finite;
  const double dmax = ln_dmax(p, ge, H, Nd, &dword);
  long long t0, t1;
  pool_range(a, t0, t1);
  if (bad) {                                               // (uniform) NaN rows; the finishing kernel writes the parameters' NaN
    const long long i1 = 2 * t1 < a.N ? 2 * t1 : a.N;
    for (long long i = 2 * t0 + threadIdx.x; i < i1; i += POOL_BLOCK) {
      if (g.g_x) g.g_x[(size_t)env * a.N + i] = nan;
      if (g.g_v) g.g_v[(size_t)env * a.N + i] = nan;
    }
    return;
  }
  const bool dep = g.want_params != 0;
  for (int k = threadIdx.x; k < H; k += POOL_BLOCK) {
#pragma unroll
    for (int m = 0; m < 6; ++m) sums[m * H + k] = 0ull;
    const LnVjpUnits ue = ln_vjp_units(p[4 * H + k], ge[k], dmax, rmx, umx, Nd, n.sqrtH, a.bitsN);
    unit[k] = dep ? ue.w : kPoolSkip;
    unit[H + k] = dep ? ue.g : kPoolSkip;
    unit[2 * H + k] = dep ? ue.b : kPoolSkip;
  }
  __syncthreads();
  const bool is_tanh = a.activation == PIC_ACT_TANH;
  const double cx = kTwoPi / a.L;
  for (long long tc = t0; tc < t1; tc += (long long)POOL_BLOCK * kPoolTiles) {
    PoolLane q;
    pool_load(a, xe, ve, tc, t1, q);
    double mu[kPoolPerLane], r[kPoolPerLane], m1[kPoolPerLane], m2[kPoolPerLane];
    ln_stats(p, H, n, q, mu, r);
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) m1[j] = m2[j] = 0.0;
    for (int k = 0; k < H; ++k) {
      const int ug = unit[H + k], ub = unit[2 * H + k];
      const bool ong = ug != kPoolSkip && ug != kPoolNan, onb = ub != kPoolSkip && ub != kPoolNan;      // (uniform)
      const LnRow w = ln_row(p, H, k);
      const double ck = ge[k];
      long long pg = 0, pb = 0;
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double nn = ln_norm(w, q.c[j], q.s[j], q.u[j], mu[j], r[j], y);
        const double dn = ln_dn(nn, ck, Nd, is_tanh), dy = dn * w.g;
        m1[j] = m1[j] + dy;
        m2[j] = m2[j] + dy * y;
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
    double sx[kPoolPerLane], sv[kPoolPerLane];
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) {
      m1[j] = m1[j] / n.Hd;
      m2[j] = m2[j] / n.Hd;
      sx[j] = sv[j] = 0.0;
    }
    for (int k = 0; k < H; ++k) {
      const int ue = unit[k];
      const bool on = ue != kPoolSkip && ue != kPoolNan;   // (uniform)
      const LnRow w = ln_row(p, H, k);
      const double ck = ge[k];
      long long pc = 0, ps = 0, pu = 0, pr = 0;
#pragma unroll
      for (int j = 0; j < kPoolPerLane; ++j) {
        double y;
        const double nn = ln_norm(w, q.c[j], q.s[j], q.u[j], mu[j], r[j], y);
        const double dy = ln_dn(nn, ck, Nd, is_tanh) * w.g;
        const double dz = ((dy - m1[j]) - y * m2[j]) * r[j];
        sx[j] = sx[j] + dz * (w.w1 * q.c[j] - w.w0 * q.s[j]);
        sv[j] = sv[j] + dz * w.w2;
        if (on && q.on[j]) {
          pc += __double2ll_rn(ldexp(dz * q.c[j], -ue));
          ps += __double2ll_rn(ldexp(dz * q.s[j], -ue));
          pu += __double2ll_rn(ldexp(dz * q.u[j], -ue));
          pr += __double2ll_rn(ldexp(dz, -ue));
        }
      }
      if (on) {
        pc = wave_sum_i64(pc);
        ps = wave_sum_i64(ps);
        pu = wave_sum_i64(pu);
        pr = wave_sum_i64(pr);
        if (lane == 0) {
          if (pc) atomicAdd(sums + k, (unsigned long long)pc);
          if (ps) atomicAdd(sums + H + k, (unsigned long long)ps);
          if (pu) atomicAdd(sums + 2 * H + k, (unsigned long long)pu);
          if (pr) atomicAdd(sums + 3 * H + k, (unsigned long long)pr);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kPoolPerLane; ++j) {
      if (!q.on[j]) continue;
      const long long i = 2 * (tc + (long long)(j >> 1) * POOL_BLOCK + threadIdx.x) + (j & 1);
      const size_t o = (size_t)env * a.N + i;
      if (g.g_x) g.g_x[o] = cx * sx[j];
      if (g.g_v) g.g_v[o] = a.v_scale * sv[j];
    }
  }
  __syncthreads();
  if (!dep) return;
  for (int c = threadIdx.x; c < 6 * H; c += POOL_BLOCK) {
    const unsigned long long s = sums[c];
    if (s) atomicAdd(a.acc + (size_t)env * 6 * H + c, s);
  }
}

// One workgroup per environment: the 6H integer sums to gE [env][6H] in the parameters' order (g_W [H][3], g_b, g_gamma, g_beta
// [H] each); +0 where the bound is zero, NaN for a non-finite bound and for an environment that is NaN as a whole; the
// accumulators and the two max words are cleared behind the read.
__global__ __launch_bounds__(POOL_BLOCK) void pool_ln_vjp_finish_kernel(PoolArgs a, PoolLnArgs n, PoolVjpArgs g, double* __restrict__ gE) {
  __shared__ unsigned long long dword;
  const int env = blockIdx.x, H = a.H;
  const unsigned long long mb = a.umax[env];
  const bool finite = mb < kMomInfBits;
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const double* __restrict__ ge = n.cot + (size_t)env * H;
  const double umx = finite ? __longlong_as_double((long long)mb) : 0.0, Nd = (double)a.N;
  const double rmx = __longlong_as_double((long long)n.rmax[env]);
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const bool bad = ln_env_bad(p, ge, H, umx) || !finite;
  const double dmax = ln_dmax(p, ge, H, Nd, &dword);
  if (g.want_params) {
    for (int c = threadIdx.x; c < 6 * H; c += POOL_BLOCK) {
      const int m = c / H, k = c - m * H;
      unsigned long long* s = a.acc + (size_t)env * 6 * H + c;
      const LnVjpUnits us = ln_vjp_units(p[4 * H + k], ge[k], dmax, rmx, umx, Nd, n.sqrtH, a.bitsN);
      const int ue = bad ? kPoolNan : (m < 4 ? us.w : (m == 4 ? us.g : us.b));
      double r = 0.0;
      if (ue == kPoolNan) r = nan;
      else if (ue != kPoolSkip) r = ldexp((double)(long long)*s, ue);
      gE[(size_t)env * 6 * H + (m < 3 ? 3 * k + m : m * H + k)] = r;
      *s = 0ull;
    }
  }
  __syncthreads();                                         // (every lane has read the max words)
  if (threadIdx.x == 0) a.umax[env] = n.rmax[env] = 0ull;
}

}  // namespace
