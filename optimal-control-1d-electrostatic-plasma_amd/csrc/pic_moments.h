// pic_moments.h -- the fluid moments of the stored particles on the handle's mesh (include/picstep.h: pic_moments*):
//   m0_j = s sum_i W_j(x_i)   m1_j = s sum_i W_j(x_i) v_i   m2_j = s sum_i W_j(x_i) v_i^2      s = n0 L / (N dx)
// with the handle's own shape function: the cell is locate<P, SHAPE>'s; the weights are the forward's for float64 particles and
// the shape function in double at the held position for the 32-bit formats (mom_weights).  All three
// deposits are 64-bit integer sums: m0 in the forward's 2^-fg units (to_fixed), m1 and m2 in units taken from the environment's
// max |v| (adj_unit_exp), so nothing depends on the grid, the schedule or the batch.  The gather of a cotangent on the moments
// back to the particles (float64 + CIC) writes dense rows or adds to the adjoint state of a tape (pic_tape_moments_cot).
// Off the step path: the kernels read the state a step left.
#pragma once
#include "pic_adjoint.h"

namespace {

constexpr unsigned long long kMomInfBits = 0x7FF0000000000000ull;   // block_max_to's mark of a non-finite velocity

struct MomArgs {
  long long N, ld;
  long long tiles_per_wg;   // 16-byte tiles (P::VEC particles) per workgroup and lane column: a workgroup's range is contiguous
  int Ng;
  int fg;                   // fractional bits of m0's units (the forward's)
  int bitsN;                // 2^bitsN >= N: headroom of the units of m1 and m2
  int num_envs;
  double magic;             // the forward's fixed-point magic (to_fixed)
  double L, dx, scale;
};

// exponent e of an environment's velocities, max |v| < 2^e (max bits finite and non-zero)
__device__ __forceinline__ int mom_vexp(unsigned long long maxbits) { return ilogb(__longlong_as_double((long long)maxbits)) + 1; }
// m2 is deposited while v^2 cannot overflow: max |v| < 2^511
__device__ __forceinline__ bool mom_m2_ok(unsigned long long maxbits) { return mom_vexp(maxbits) <= 511; }

// The weights the moments deposit with, in double.  float64 particles: the forward's own weights (m0 is the forward's density bit
// for bit).  The 32-bit formats: the forward's CELL (the same float32 floor, resp. the high word of u Ng), and the shape function
// evaluated in double at the offset d of the held position in that cell, d = x / dx - jf (resp. frac 2^-32, exact).  The
// forward's float32 weights would not do: ((j + 1) dx - x) / dx near x = L carries the rounding of a float32 at L divided by
// dx, the same for every particle of a cell (1e-5 of the density at L = 50, Ng = 250).
template <typename P, int SHAPE>
__device__ __forceinline__ void mom_weights(typename P::X xw, const Consts<P>& k, const typename P::W (&w)[3], unsigned frac,
                                            double dx, double (&out)[3]) {
  if constexpr (sizeof(typename P::W) == 8) {
    out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
  } else {
    double d;
    if constexpr (P::kFixed) {
      d = (double)frac * 2.3283064365386963e-10;           // 2^-32
    } else {
      const float jf = floor(div_dx(xw, k.dx, k.rdx));     // locate_in_box's cell, before its fold
      d = (double)xw / dx - (double)jf;
    }
    if (SHAPE == PIC_CIC) {
      out[0] = 1.0 - d; out[1] = d; out[2] = 0.0;
    } else {
      const double a = 1.5 - d, b = d - 1.0, c = d - 0.5;
      out[0] = 0.5 * (a * a); out[1] = 0.75 - b * b; out[2] = 0.5 * (c * c);
    }
  }
}

// Per-environment max |v| as the bit pattern of a non-negative double into vmax[env] (zero before; a non-finite velocity
// saturates it at kMomInfBits).  One read of v; grid (workgroups per environment, environments), the deposit's ranges.
template <typename P>
__global__ __launch_bounds__(BLOCK) void moments_max_kernel(const typename P::V* __restrict__ v, unsigned long long* __restrict__ vmax,
                                                            MomArgs a) {
  using VV = typename P::VV;
  constexpr int VEC = P::VEC;
  const int env = blockIdx.y;
  const VV* vv = reinterpret_cast<const VV*>(v + (size_t)env * a.ld);
  const long long ntiles = (a.N + VEC - 1) / VEC;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_wg * BLOCK;
  long long t1 = t0 + a.tiles_per_wg * BLOCK;
  t1 = t1 < ntiles ? t1 : ntiles;
  unsigned long long mb = 0ull;
  for (long long t = t0 + threadIdx.x; t < t1; t += BLOCK) {
    const VV vt = stream_load(vv + t);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (t * VEC + k >= a.N) break;
      const double av = fabs((double)vt[k]);
      unsigned long long b = (unsigned long long)__double_as_longlong(av);
      if (!(av <= 1.7976931348623157e308)) b = kMomInfBits;
      mb = b > mb ? b : mb;
    }
  }
  block_max_to(__longlong_as_double((long long)mb), vmax + env);
}

// Deposit pass: grid (workgroups per environment, environments).  Three LDS meshes of Ng + 2 words (CIC uses Ng + 1 of them: the
// right node of the last cell is slot Ng; TSC slot s is node s - 1), cleared under the latency of the first loads; the
// workgroup reads its particle range once and adds three integers per touched node (ds_add_u64), then flushes one memory-side
// atomic per non-zero node and moment into acc [3][env][Ng].  m1 and m2 are skipped in an environment whose velocities are all
// zero or not all finite (the finishing kernel writes +0 / NaN there), m2 also where v^2 could overflow.
template <typename P, int SHAPE>
__global__ __launch_bounds__(BLOCK) void moments_deposit_kernel(const typename P::X* __restrict__ x, const typename P::V* __restrict__ v,
                                                                const unsigned long long* __restrict__ vmax,
                                                                unsigned long long* __restrict__ acc, MomArgs a) {
  using XV = typename P::XV;
  using VV = typename P::VV;
  constexpr int VEC = P::VEC;
  constexpr int OFF = (SHAPE == PIC_TSC) ? 1 : 0;
  constexpr int NW = (SHAPE == PIC_TSC) ? 3 : 2;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.y, Ng = a.Ng, stride = Ng + 2;
  const XV* xv = reinterpret_cast<const XV*>(x + (size_t)env * a.ld);
  const VV* vv = reinterpret_cast<const VV*>(v + (size_t)env * a.ld);
  const long long ntiles = (a.N + VEC - 1) / VEC;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_wg * BLOCK;
  long long t1 = t0 + a.tiles_per_wg * BLOCK;
  t1 = t1 < ntiles ? t1 : ntiles;
  long long t = t0 + threadIdx.x;
  bool have = t < t1;
  XV xn{};
  VV vn{};
  if (have) {
    xn = stream_load(xv + t);
    vn = stream_load(vv + t);
  }
  for (int c = threadIdx.x; c < 3 * stride; c += BLOCK) lds[c] = 0ull;
  const unsigned long long mb = vmax[env];
  const bool dep1 = mb != 0ull && mb < kMomInfBits;
  const bool dep2 = dep1 && mom_m2_ok(mb);
  const int u1 = adj_unit_exp(mb, a.bitsN);                // max |v| < 2^e: units 2^(e + bitsN - 61) and 2^(2e + bitsN - 61)
  const int u2 = dep1 ? u1 + mom_vexp(mb) : 0;
  __syncthreads();
  const Consts<P> kc(a.L, a.dx, Ng);
  unsigned long long* l0 = lds;
  unsigned long long* l1 = lds + stride;
  unsigned long long* l2 = lds + 2 * stride;
  unsigned bad = 0u;
  while (have) {
    const XV xt = xn;
    const VV vt = vn;
    const long long tc = t;
    t += BLOCK;
    have = t < t1;
    if (have) {
      xn = stream_load(xv + t);
      vn = stream_load(vv + t);
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (tc * VEC + k >= a.N) break;
      typename P::X xw;
      typename P::W w[3];
      int j;
      unsigned frac;
      locate<P, SHAPE>(xt[k], kc, xw, j, w, frac, bad);
      double wq[3];
      mom_weights<P, SHAPE>(xw, kc, w, frac, a.dx, wq);
      const double vd = (double)vt[k];
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const double wd = wq[q];
        atomicAdd(l0 + j + q, (unsigned long long)to_fixed(wd, a.magic));
        if (dep1) {
          const double wv = wd * vd;
          atomicAdd(l1 + j + q, (unsigned long long)__double2ll_rn(ldexp(wv, -u1)));
          if (dep2) atomicAdd(l2 + j + q, (unsigned long long)__double2ll_rn(ldexp(wv * vd, -u2)));
        }
      }
    }
  }
  (void)bad;                                               // (the state's bad positions are the sweeps' to count)
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    if ((m == 1 && !dep1) || (m == 2 && !dep2)) continue;
    const unsigned long long* lm = lds + m * stride;
    unsigned long long* out = acc + ((size_t)m * a.num_envs + env) * Ng;
    for (int c = threadIdx.x; c < Ng; c += BLOCK) {
      unsigned long long s = lm[c + OFF];
      if (SHAPE == PIC_CIC) {
        if (c == 0) s += lm[Ng];
      } else {
        if (c == 0) s += lm[Ng + 1];
        if (c == Ng - 1) s += lm[0];
      }
      if (s) atomicAdd(out + c, s);
    }
  }
}

// One workgroup per environment: the integer sums to m [env][3][Ng] (m0 by solve_environment's expression for n), +0 in m1 and
// m2 of an environment at rest, NaN where a velocity is not finite (+inf in m2 where v^2 could overflow); the accumulators and
// the environment's max word are cleared behind the read.
__global__ __launch_bounds__(BLOCK) void moments_finish_kernel(unsigned long long* __restrict__ acc, unsigned long long* __restrict__ vmax,
                                                               double* __restrict__ m, MomArgs a) {
  const int env = blockIdx.x, Ng = a.Ng;
  const unsigned long long mb = vmax[env];
  const bool finite = mb < kMomInfBits, dep1 = mb != 0ull && finite, dep2 = dep1 && mom_m2_ok(mb);
  const int u1 = adj_unit_exp(mb, a.bitsN);
  const int u2 = dep1 ? u1 + mom_vexp(mb) : 0;
  const double unit0 = ldexp(1.0, -a.fg);
  const double nan = __longlong_as_double(0x7FF8000000000000ll), inf = __longlong_as_double((long long)kMomInfBits);
  unsigned long long* a0 = acc + ((size_t)0 * a.num_envs + env) * Ng;
  unsigned long long* a1 = acc + ((size_t)1 * a.num_envs + env) * Ng;
  unsigned long long* a2 = acc + ((size_t)2 * a.num_envs + env) * Ng;
  double* out = m + (size_t)env * 3 * Ng;
  for (int j = threadIdx.x; j < Ng; j += BLOCK) {
    out[j] = ((double)(long long)a0[j] * unit0) * a.scale;
    double m1 = 0.0, m2 = 0.0;
    if (dep1) m1 = ldexp((double)(long long)a1[j], u1) * a.scale;
    if (dep2) m2 = ldexp((double)(long long)a2[j], u2) * a.scale;
    else if (dep1) m2 = inf;
    if (!finite) m1 = m2 = nan;
    out[Ng + j] = m1;
    out[2 * Ng + j] = m2;
    a0[j] = 0ull;
    a1[j] = 0ull;
    a2[j] = 0ull;
  }
  __syncthreads();                                         // (every lane has read the max word)
  if (threadIdx.x == 0) vmax[env] = 0ull;
}

// The gather: one thread per particle (float64, CIC), the derivative of sum_kj g[k][j] m_k,j by x_i and v_i with the unquantised
// weights (DESIGN.md 7c's almost-everywhere derivative):
//   d_x = s (slope(g0) + v slope(g1) + v^2 slope(g2)),  d_v = s ((w_l g1[j] + w_r g1[jr]) + 2 v (w_l g2[j] + w_r g2[jr]))
// x, v [env][ld]; g [env][3][Ng]; ox, ov rows of `orow` elements: overwritten (dense [env][N], pic_moments_vjp), or added to (the
// adjoint state [env][ld] of a tape, pic_tape_moments_cot).  Grid (N / BLOCK, environments).
template <bool ADD>
__global__ __launch_bounds__(BLOCK) void moments_vjp_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                            const double* __restrict__ g, MomArgs a, double* __restrict__ ox,
                                                            double* __restrict__ ov, long long orow) {
  const int env = blockIdx.y, Ng = a.Ng;
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.N) return;
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const double xs = x[(size_t)env * a.ld + i], vs = v[(size_t)env * a.ld + i];
  double w[3], xw;
  int j, jr;
  unsigned bad = 0u;
  adj_locate(xs, k, xw, j, jr, w, bad);
  const double* g0 = g + (size_t)env * 3 * Ng;
  const double* g1 = g0 + Ng;
  const double* g2 = g1 + Ng;
  const double dx = a.scale * (slope_dot(g0, j, jr, a.dx) + vs * slope_dot(g1, j, jr, a.dx) + (vs * vs) * slope_dot(g2, j, jr, a.dx));
  const double dv = a.scale * ((w[0] * g1[j] + w[1] * g1[jr]) + (2.0 * vs) * (w[0] * g2[j] + w[1] * g2[jr]));
  const size_t o = (size_t)env * orow + i;
  if (ADD) {
    ox[o] = ox[o] + dx;
    ov[o] = ov[o] + dv;
  } else {
    ox[o] = dx;
    ov[o] = dv;
  }
  (void)bad;
}

}  // namespace
