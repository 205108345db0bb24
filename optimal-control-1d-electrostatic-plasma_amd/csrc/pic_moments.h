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
#include "pic_phase.h"      // pic_v2d_a8: a tangent tile of dense rows that start on 8 bytes only (N odd)

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

// ---------------------------------------------------------------------------------------------
// Forward mode (pic_moments_jvp, pic_tape_tangent_moments): the directional derivative of the three moments along
// tangents (dx_i, dv_i) of the particles, float64 + CIC, with the almost-everywhere derivative of the gather above (weight slopes
// -/+ 1/dx).  With iota = dx_i / dx a particle adds to its left node j and its right node jr
//   dm0:  -iota                         +iota
//   dm1:  w_l dv - iota v               w_r dv + iota v
//   dm2:  2 w_l v dv - iota v^2         2 w_r v dv + iota v^2
// (times s): term by term the transpose of moments_vjp_kernel.  Every term is rounded to a 64-bit integer in a unit taken from the
// max of a bound on one term per (moment, direction, environment), so the sums do not depend on their order.
// ---------------------------------------------------------------------------------------------
struct MomJvpArgs {
  const double* dx;            // direction 0, environment 0 of the x tangents, or null (0)
  const double* dv;            // the same of the v tangents
  long long dstride;           // elements from one direction to the next
  long long erow;              // elements from one environment's row to the next (ld of the tangent state, N of dense rows)
  unsigned long long* acc;     // [3][K][env][Ng] integer sums, zero between uses
  unsigned long long* umax;    // [3][K][env] bit patterns of the terms' bounds, zero between uses
  int K;                       // directions
  int kd;                      // directions a deposit workgroup holds in LDS (grid z: groups of kd)
};

// tile t (particles 2t, 2t + 1) of a tangent row, or zeros for a null row; the odd last particle of a row is read alone, so nothing
// beyond N is ever read
__device__ __forceinline__ pic_v2d mom_tan_tile(const double* __restrict__ row, long long t, bool pair) {
  pic_v2d r = {0.0, 0.0};
  if (row) {
    if (pair) {
      const pic_v2d_a8 q = stream_load(reinterpret_cast<const pic_v2d_a8*>(row + 2 * t));
      r[0] = q[0]; r[1] = q[1];
    } else {
      r[0] = row[2 * t];
    }
  }
  return r;
}

// running max of bounds as bit patterns (ordered like the non-negative values); a non-finite bound saturates it for good
__device__ __forceinline__ void mom_max_bits(unsigned long long& m, double bound) {
  unsigned long long b = (unsigned long long)__double_as_longlong(bound);
  if (!(bound <= 1.7976931348623157e308)) b = kMomInfBits;
  m = b > m ? b : m;
}

__device__ __forceinline__ unsigned long long* mom_jvp_word(const MomJvpArgs& j, int m, int d, int num_envs, int env) {
  return j.umax + ((size_t)m * j.K + d) * num_envs + env;
}

// Max pass: grid (workgroups per environment, environments), the deposit's ranges.  One read of v and of every direction's dx, dv;
// per (moment, direction, environment) the max of a bound on one deposited term,
//   b0 = |iota|   b1 = |dv| + |iota v|   b2 = 2 |v dv| + |iota| v^2
// through block_max_to (order-free; a non-finite value saturates the word).
template <int KD>
__global__ __launch_bounds__(BLOCK) void moments_jvp_max_kernel(const double* __restrict__ v, MomArgs a, MomJvpArgs j) {
  const int env = blockIdx.y;
  const pic_v2d* vv = reinterpret_cast<const pic_v2d*>(v + (size_t)env * a.ld);
  const long long ntiles = (a.N + 1) / 2;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_wg * BLOCK;
  long long t1 = t0 + a.tiles_per_wg * BLOCK;
  t1 = t1 < ntiles ? t1 : ntiles;
  const size_t drow = (size_t)env * j.erow;
  unsigned long long m0[KD], m1[KD], m2[KD];
#pragma unroll
  for (int d = 0; d < KD; ++d) m0[d] = m1[d] = m2[d] = 0ull;
  for (long long t = t0 + threadIdx.x; t < t1; t += BLOCK) {
    const bool pair = 2 * t + 1 < a.N;
    const pic_v2d vt = stream_load(vv + t);
#pragma unroll
    for (int d = 0; d < KD; ++d) {
      if (d >= j.K) break;
      const size_t o = (size_t)d * j.dstride + drow;
      const pic_v2d xd = mom_tan_tile(j.dx ? j.dx + o : nullptr, t, pair);
      const pic_v2d vd = mom_tan_tile(j.dv ? j.dv + o : nullptr, t, pair);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k == 1 && !pair) break;
        const double vs = vt[k], io = fabs(xd[k] / a.dx);
        mom_max_bits(m0[d], io);
        mom_max_bits(m1[d], fabs(vd[k]) + fabs(io * vs));
        mom_max_bits(m2[d], 2.0 * fabs(vs * vd[k]) + io * (vs * vs));
      }
    }
  }
#pragma unroll
  for (int d = 0; d < KD; ++d) {
    if (d >= j.K) break;
    block_max_to(__longlong_as_double((long long)m0[d]), mom_jvp_word(j, 0, d, a.num_envs, env));
    block_max_to(__longlong_as_double((long long)m1[d]), mom_jvp_word(j, 1, d, a.num_envs, env));
    block_max_to(__longlong_as_double((long long)m2[d]), mom_jvp_word(j, 2, d, a.num_envs, env));
  }
}

// Deposit pass: grid (workgroups per environment, environments, groups of kd <= KD directions).  LDS [kd][3][Ng + 1] 64-bit
// words (the right node of the last cell is slot Ng), cleared under the latency of the first tile's loads.  x, v and the group's
// dx, dv are read once in 16-byte tiles, the next tile requested before the current one is deposited; cell, weights, v and v^2
// are computed once per particle and serve every direction.  dm0 adds -r and +r of one rounded r: its integer sum is zero.  A
// (moment, direction) whose max word is zero or saturated is skipped (the finishing kernel writes +0 / NaN there).  The flush is
// one memory-side atomic per non-zero node.
template <int KD>
__global__ __launch_bounds__(BLOCK) void moments_jvp_deposit_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                                    MomArgs a, MomJvpArgs j) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.y, Ng = a.Ng, stride = Ng + 1, d0 = blockIdx.z * j.kd;
  const int nd = min(j.kd, j.K - d0);
  const pic_v2d* xv = reinterpret_cast<const pic_v2d*>(x + (size_t)env * a.ld);
  const pic_v2d* vv = reinterpret_cast<const pic_v2d*>(v + (size_t)env * a.ld);
  const long long ntiles = (a.N + 1) / 2;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_wg * BLOCK;
  long long t1 = t0 + a.tiles_per_wg * BLOCK;
  t1 = t1 < ntiles ? t1 : ntiles;
  const size_t drow = (size_t)d0 * j.dstride + (size_t)env * j.erow;
  const double* tx = j.dx ? j.dx + drow : nullptr;
  const double* tv = j.dv ? j.dv + drow : nullptr;
  long long t = t0 + threadIdx.x;
  bool have = t < t1;
  pic_v2d xn = {0.0, 0.0}, vn = {0.0, 0.0}, dxn[KD], dvn[KD];
#pragma unroll
  for (int d = 0; d < KD; ++d) dxn[d] = dvn[d] = pic_v2d{0.0, 0.0};
  if (have) {
    const bool pair = 2 * t + 1 < a.N;
    xn = stream_load(xv + t);
    vn = stream_load(vv + t);
#pragma unroll
    for (int d = 0; d < KD; ++d) {
      if (d >= nd) break;
      dxn[d] = mom_tan_tile(tx ? tx + (size_t)d * j.dstride : nullptr, t, pair);
      dvn[d] = mom_tan_tile(tv ? tv + (size_t)d * j.dstride : nullptr, t, pair);
    }
  }
  for (int c = threadIdx.x; c < nd * 3 * stride; c += BLOCK) lds[c] = 0ull;
  int ue[3][KD];
  bool on[3][KD];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int d = 0; d < KD; ++d) {
      const unsigned long long mb = d < nd ? *mom_jvp_word(j, m, d0 + d, a.num_envs, env) : 0ull;
      on[m][d] = mb != 0ull && mb < kMomInfBits;
      ue[m][d] = adj_unit_exp(mb, a.bitsN);
    }
  }
  __syncthreads();
  const Consts<PosF64> kc(a.L, a.dx, Ng);
  unsigned bad = 0u;
  while (have) {
    const pic_v2d xt = xn, vt = vn;
    pic_v2d dxt[KD], dvt[KD];
#pragma unroll
    for (int d = 0; d < KD; ++d) { dxt[d] = dxn[d]; dvt[d] = dvn[d]; }
    const long long tc = t;
    t += BLOCK;
    have = t < t1;
    if (have) {
      const bool pair = 2 * t + 1 < a.N;
      xn = stream_load(xv + t);
      vn = stream_load(vv + t);
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (d >= nd) break;
        dxn[d] = mom_tan_tile(tx ? tx + (size_t)d * j.dstride : nullptr, t, pair);
        dvn[d] = mom_tan_tile(tv ? tv + (size_t)d * j.dstride : nullptr, t, pair);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (2 * tc + k >= a.N) break;
      double w[3], xw;
      int jl, jr;
      adj_locate(xt[k], kc, xw, jl, jr, w, bad);
      const double vs = vt[k], v2 = vs * vs;
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (d >= nd) break;
        unsigned long long* l0 = lds + (size_t)d * 3 * stride + jl;
        const double io = dxt[d][k] / a.dx, dvs = dvt[d][k];
        if (on[0][d]) {
          const long long r = __double2ll_rn(ldexp(io, -ue[0][d]));
          atomicAdd(l0, (unsigned long long)(-r));
          atomicAdd(l0 + 1, (unsigned long long)r);
        }
        if (on[1][d]) {
          const double iv = io * vs;
          atomicAdd(l0 + stride, (unsigned long long)__double2ll_rn(ldexp(w[0] * dvs - iv, -ue[1][d])));
          atomicAdd(l0 + stride + 1, (unsigned long long)__double2ll_rn(ldexp(w[1] * dvs + iv, -ue[1][d])));
        }
        if (on[2][d]) {
          const double iv2 = io * v2, vdv = 2.0 * (vs * dvs);
          atomicAdd(l0 + 2 * stride, (unsigned long long)__double2ll_rn(ldexp(w[0] * vdv - iv2, -ue[2][d])));
          atomicAdd(l0 + 2 * stride + 1, (unsigned long long)__double2ll_rn(ldexp(w[1] * vdv + iv2, -ue[2][d])));
        }
      }
    }
  }
  (void)bad;                                               // (the state's bad positions are the sweeps' to count)
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 3; ++m) {
#pragma unroll
    for (int d = 0; d < KD; ++d) {
      if (d >= nd) break;
      if (!on[m][d]) continue;
      const unsigned long long* lm = lds + ((size_t)d * 3 + m) * stride;
      unsigned long long* out = j.acc + (((size_t)m * j.K + d0 + d) * a.num_envs + env) * Ng;
      for (int c = threadIdx.x; c < Ng; c += BLOCK) {
        unsigned long long s = lm[c];
        if (c == 0) s += lm[Ng];
        if (s) atomicAdd(out + c, s);
      }
    }
  }
}

// One workgroup per (environment, direction): integers x unit x s into out[d * out_dstride + (env 3 + m) Ng + node]; +0 in a
// moment whose max word is zero, NaN in one whose max word is saturated (that moment of that direction of that environment only);
// the accumulators and the three max words are cleared behind the read.
__global__ __launch_bounds__(BLOCK) void moments_jvp_finish_kernel(MomArgs a, MomJvpArgs j, double* __restrict__ out,
                                                                   long long out_dstride) {
  const int env = blockIdx.x, d = blockIdx.y, Ng = a.Ng;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  double* o = out + (size_t)d * out_dstride + (size_t)env * 3 * Ng;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const unsigned long long mb = *mom_jvp_word(j, m, d, a.num_envs, env);
    const bool finite = mb < kMomInfBits, dep = mb != 0ull && finite;
    const int ue = adj_unit_exp(mb, a.bitsN);
    unsigned long long* am = j.acc + (((size_t)m * j.K + d) * a.num_envs + env) * Ng;
    for (int c = threadIdx.x; c < Ng; c += BLOCK) {
      double r = 0.0;
      if (dep) r = ldexp((double)(long long)am[c], ue) * a.scale;
      if (!finite) r = nan;
      o[(size_t)m * Ng + c] = r;
      am[c] = 0ull;
    }
  }
  __syncthreads();                                         // (every lane has read the max words)
  if (threadIdx.x < 3) *mom_jvp_word(j, threadIdx.x, d, a.num_envs, env) = 0ull;
}

}  // namespace
