// pic_phase.h -- the smoothed phase-space density and its KL cost (include/picstep.h: pic_phase_kl_smooth*):
// an integer CIC deposit of every environment's particles on an nx x nv grid over [0, L] x [vmin, vmax], a per-environment
// finishing kernel (density, KL against a target, the cotangent grid of the KL) and the gather of that grid back to the particles
// (into dense rows, or added to the adjoint state of a tape: DESIGN.md 7h; or dotted with tangents of the particles, the forward
// mode: DESIGN.md 7j).
// Float64 particles only.  Off the step path: the kernels read the state a step left.
#pragma once
#include "pic_device.h"

namespace {

constexpr int kPhaseLdsBytes = 64 << 10;      // LDS of a deposit workgroup: its band of grid rows as int64 sums
constexpr int kPhaseMaxBins = 1024;           // bins per axis

struct PhaseArgs {
  long long N, ld;
  long long tiles_per_wg;   // 16-byte tiles (two particles) per workgroup and lane column: a workgroup's range is contiguous
  int nx, nv;
  int rows;                 // grid rows (x bins) per band: rows * nv int64 fit in kPhaseLdsBytes
  int abits, bbits;         // fractional bits of the x and v weights; a particle is 2^(abits + bbits) units
  double L, vmin, vmax;
  double rdx, rdv;          // 1 / dx and 1 / dv, rounded once on the host: bins are located by multiplication
};

// Bins and CIC fractions of one particle: x periodic on the bin centres (i + 1/2) dx, v on vmin + (j + 1/2) dv with the outer
// half-bins clamped to the edge bin (fv = 0, vslope false).  false: outside [0, L] x [vmin, vmax] (or not finite), dropped as
// np.histogram2d drops it.  Every index returned lies in its axis's range.
__device__ __forceinline__ bool phase_locate(double x, double v, const PhaseArgs& a, int& i0, int& i1, int& j0, int& j1,
                                             double& fx, double& fv, bool& vslope) {
  if (!(x >= 0.0 && x <= a.L && v >= a.vmin && v <= a.vmax)) return false;
  const double u = x * a.rdx - 0.5;
  const double fu = floor(u);
  fx = u - fu;
  i0 = (int)fu;                                 // -1 .. nx-1
  i1 = i0 + 1;
  if (i0 < 0) i0 += a.nx;
  if (i1 >= a.nx) i1 -= a.nx;
  i0 = min(max(i0, 0), a.nx - 1);
  i1 = min(max(i1, 0), a.nx - 1);
  const double w = (v - a.vmin) * a.rdv - 0.5;
  vslope = false;
  fv = 0.0;
  if (w < 0.0) {
    j0 = j1 = 0;
  } else {
    const double fw = floor(w);
    j0 = (int)fw;
    if (j0 >= a.nv - 1) {
      j0 = j1 = a.nv - 1;
    } else {
      j1 = j0 + 1;
      fv = w - fw;
      vslope = true;
    }
  }
  return true;
}

// Deposit pass: grid (workgroups per environment, bands, environments).  Band b holds grid rows [b rows, (b + 1) rows) in LDS;
// its workgroups read their particle range once and add the integer weights that fall into it (ds_add_u64), then flush one
// memory-side atomic per non-zero bin into acc [env][nx][nv].  Integer sums: the result does not depend on the grid.
__global__ __launch_bounds__(BLOCK) void phase_deposit_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                              unsigned long long* __restrict__ acc, PhaseArgs a) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* h = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.z;
  const int r0 = blockIdx.y * a.rows;
  const int r1 = min(r0 + a.rows, a.nx);
  const int words = (r1 - r0) * a.nv;
  for (int i = threadIdx.x; i < words; i += BLOCK) h[i] = 0ull;
  __syncthreads();
  const unsigned long long ua = 1ull << a.abits, ub = 1ull << a.bbits;
  const double sa = (double)ua, sb = (double)ub;
  const pic_v2d* xv = reinterpret_cast<const pic_v2d*>(x + (size_t)env * a.ld);
  const pic_v2d* vv = reinterpret_cast<const pic_v2d*>(v + (size_t)env * a.ld);
  const long long ntiles = (a.N + 1) / 2;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_wg * BLOCK;
  long long t1 = t0 + a.tiles_per_wg * BLOCK;
  t1 = t1 < ntiles ? t1 : ntiles;
  for (long long t = t0 + threadIdx.x; t < t1; t += BLOCK) {
    const pic_v2d xt = stream_load(xv + t);
    const pic_v2d vt = stream_load(vv + t);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (t * 2 + k >= a.N) break;
      int i0, i1, j0, j1;
      double fx, fv;
      bool vs;
      if (!phase_locate(xt[k], vt[k], a, i0, i1, j0, j1, fx, fv, vs)) continue;
      const unsigned long long ax = (unsigned long long)rint(fx * sa), av = (unsigned long long)rint(fv * sb);
      const unsigned long long wx[2] = {ua - ax, ax}, wv[2] = {ub - av, av};
      const int ii[2] = {i0, i1}, jj[2] = {j0, j1};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        if (ii[p] < r0 || ii[p] >= r1) continue;
        const int r = ii[p] - r0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const unsigned long long w = wx[p] * wv[q];
          if (w) atomicAdd(&h[r * a.nv + jj[q]], w);
        }
      }
    }
  }
  __syncthreads();
  unsigned long long* g = acc + ((size_t)env * a.nx + r0) * a.nv;
  for (int i = threadIdx.x; i < words; i += BLOCK) {
    const unsigned long long c = h[i];
    if (c) atomicAdd(&g[i], c);
  }
}

struct PhaseFinishArgs {
  unsigned long long* acc;   // [env][nb2] integer sums (cleared here behind the read)
  int nb2;
  double unit, norm, dxdv;   // f = ((double)sum * unit) * norm, unit = 2^-(abits + bbits), norm = n0 / dx / dv / N
  const double* feq;         // [nb2] or [env][nb2] (feq_stride = nb2), or null
  long long feq_stride;
  const double* d_kl;        // [env] cotangents of the KL (read when g is wanted)
  double* f;                 // [env][nb2] the density, or null
  double* kl;                // [env], or null (needs feq)
  double* g;                 // [env][nb2] d_kl dKL/df, or null (needs feq)
};

// One workgroup per environment; the KL in a fixed order (the threads' strided partial sums, then block_sum's).
__global__ __launch_bounds__(BLOCK) void phase_finish_kernel(PhaseFinishArgs a) {
  __shared__ double ws[WAVES];
  const int env = blockIdx.x;
  const size_t row = (size_t)env * a.nb2;
  unsigned long long* c = a.acc + row;
  const double* feq = a.feq ? a.feq + (size_t)env * a.feq_stride : nullptr;
  const double d = a.g ? a.d_kl[env] : 0.0;
  double k = 0.0;
  for (int i = threadIdx.x; i < a.nb2; i += BLOCK) {
    const double f = ((double)c[i] * a.unit) * a.norm;
    c[i] = 0ull;
    if (a.f) a.f[row + i] = f;
    if (feq) {
      double gi = 0.0;
      if (f > 0.0) {
        const double r = log(f / (feq[i] + 1e-12));
        k += f * r;
        gi = d * ((r + 1.0) * a.dxdv);
      }
      if (a.g) a.g[row + i] = gi;
    }
  }
  if (a.kl) {
    const double K = block_sum<WAVES>(k, ws);
    if (threadIdx.x == 0) a.kl[env] = K * a.dxdv;
  }
}

// dKL/dx and dKL/dv of one particle against an environment's cotangent grid gr [nx][nv]: the four bins of phase_locate with the
// slopes of the unquantised CIC weights (cx = norm / dx, cv = norm / dv); 0 for a dropped particle, 0 in v in a clamped half-bin.
__device__ __forceinline__ void phase_gather(double xs, double vs, const double* __restrict__ gr, const PhaseArgs& a, double cx,
                                             double cv, double& dx, double& dv) {
  int i0, i1, j0, j1;
  double fx, fv;
  bool vsl;
  dx = 0.0;
  dv = 0.0;
  if (phase_locate(xs, vs, a, i0, i1, j0, j1, fx, fv, vsl)) {
    const double g00 = gr[(size_t)i0 * a.nv + j0], g01 = gr[(size_t)i0 * a.nv + j1];
    const double g10 = gr[(size_t)i1 * a.nv + j0], g11 = gr[(size_t)i1 * a.nv + j1];
    dx = cx * ((g10 - g00) * (1.0 - fv) + (g11 - g01) * fv);
    if (vsl) dv = cv * ((g01 - g00) * (1.0 - fx) + (g11 - g10) * fx);
  }
}

// The gather: one thread per particle, dKL/dx and dKL/dv of the unquantised CIC weights against g (cx = norm / dx,
// cv = norm / dv), into dense rows gx, gv [env][N].
__global__ __launch_bounds__(BLOCK) void phase_vjp_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                          const double* __restrict__ g, PhaseArgs a, double cx, double cv,
                                                          double* __restrict__ gx, double* __restrict__ gv) {
  const int env = blockIdx.y;
  const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= a.N) return;
  const double xs = x[(size_t)env * a.ld + i], vs = v[(size_t)env * a.ld + i];
  double dx, dv;
  phase_gather(xs, vs, g + (size_t)env * a.nx * a.nv, a, cx, cv, dx, dv);
  gx[(size_t)env * a.N + i] = dx;
  gv[(size_t)env * a.N + i] = dv;
}

// The same gather added to the adjoint state of a taped rollout (pic_tape_kl_cot): lx, lv [env][ld] +=
// dKL/dx, dKL/dv at the replayed particles x, v [env][ld].  One 16-byte tile (two particles) per lane, as the deposit reads
// them (rows start on 16 bytes: ld is even); the odd last particle of a row goes alone, so the padding is never written.
// Grid: (tiles / BLOCK, environments).
__global__ __launch_bounds__(BLOCK) void phase_vjp_add_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                              const double* __restrict__ g, PhaseArgs a, double cx, double cv,
                                                              double* __restrict__ lx, double* __restrict__ lv) {
  const int env = blockIdx.y;
  const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
  const long long i = 2 * t;
  if (i >= a.N) return;
  const size_t row = (size_t)env * a.ld;
  const double* gr = g + (size_t)env * a.nx * a.nv;
  if (i + 1 < a.N) {
    const pic_v2d xt = stream_load(reinterpret_cast<const pic_v2d*>(x + row) + t);
    const pic_v2d vt = stream_load(reinterpret_cast<const pic_v2d*>(v + row) + t);
    pic_v2d* px = reinterpret_cast<pic_v2d*>(lx + row) + t;
    pic_v2d* pv = reinterpret_cast<pic_v2d*>(lv + row) + t;
    pic_v2d ax = *px, av = *pv;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double dx, dv;
      phase_gather(xt[k], vt[k], gr, a, cx, cv, dx, dv);
      ax[k] = ax[k] + dx;
      av[k] = av[k] + dv;
    }
    *px = ax;
    *pv = av;
  } else {
    double dx, dv;
    phase_gather(x[row + i], v[row + i], gr, a, cx, cv, dx, dv);
    lx[row + i] = lx[row + i] + dx;
    lv[row + i] = lv[row + i] + dv;
  }
}

// ---------------------------------------------------------------------------------------------
// Forward mode (pic_phase_kl_smooth_jvp, pic_tape_tangent_kl): dKL~ = sum_k dKL~/dx_k dx_k + dKL~/dv_k dv_k per
// environment and direction, with phase_gather's dKL~/d(x, v) against the grid g the finishing kernel wrote for unit cotangents.
// ---------------------------------------------------------------------------------------------
constexpr int kJvpTilesPerLane = 8;                          // tiles a lane sums: a chunk is BLOCK * 8 tiles = 8192 particles,
constexpr long long kJvpChunkTiles = (long long)BLOCK * kJvpTilesPerLane;   // whatever the grid, the batch or the schedule

// a direction's tile: rows of the dense [K][env][N] layout start on 8 bytes only (N odd)
typedef double pic_v2d_a8 __attribute__((ext_vector_type(2), aligned(8)));

struct PhaseJvpArgs {
  const double* dx;       // direction 0, environment 0 of the x tangents, or null (0)
  const double* dv;       // the same of the v tangents
  long long dstride;      // elements from one direction to the next
  long long erow;         // elements from one environment's row to the next (ld of the tangent state, N of dense rows)
  double* part;           // [K][env][chunks] the chunks' sums
  int K, num_envs, chunks;
};

// Chunk c of an environment: tiles [c, c + 1) kJvpChunkTiles of its particles x, v [env][ld].  A lane sums its tiles c0 + lane,
// c0 + lane + BLOCK, ... in that order (within a tile particle 0, then particle 1; the odd last particle of a row alone, so the
// padding is never read), block_sum adds the lanes, and part[d][env][c] receives direction d's sum: one value per chunk that
// depends on the particles and the tangents alone.  phase_gather runs once per particle and serves all KD >= K directions.
// Grid: (chunks, environments).
template <int KD>
__global__ __launch_bounds__(BLOCK) void phase_jvp_kernel(const double* __restrict__ x, const double* __restrict__ v,
                                                          const double* __restrict__ g, PhaseArgs a, double cx, double cv,
                                                          PhaseJvpArgs j) {
  __shared__ double ws[WAVES];
  const int env = blockIdx.y;
  const size_t row = (size_t)env * a.ld;
  const size_t drow = (size_t)env * j.erow;
  const double* gr = g + (size_t)env * a.nx * a.nv;
  const long long ntiles = (a.N + 1) / 2;
  const long long c0 = (long long)blockIdx.x * kJvpChunkTiles;
  double s[KD];
#pragma unroll
  for (int d = 0; d < KD; ++d) s[d] = 0.0;
#pragma unroll 2
  for (int q = 0; q < kJvpTilesPerLane; ++q) {
    const long long t = c0 + (long long)q * BLOCK + threadIdx.x;
    if (t >= ntiles) break;
    const long long i = 2 * t;
    if (i + 1 < a.N) {
      const pic_v2d xt = stream_load(reinterpret_cast<const pic_v2d*>(x + row) + t);
      const pic_v2d vt = stream_load(reinterpret_cast<const pic_v2d*>(v + row) + t);
      double gx[2], gv[2];
      phase_gather(xt[0], vt[0], gr, a, cx, cv, gx[0], gv[0]);
      phase_gather(xt[1], vt[1], gr, a, cx, cv, gx[1], gv[1]);
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (d >= j.K) break;
        const size_t o = (size_t)d * j.dstride + drow + i;
        pic_v2d_a8 dxt = {0.0, 0.0}, dvt = {0.0, 0.0};
        if (j.dx) dxt = stream_load(reinterpret_cast<const pic_v2d_a8*>(j.dx + o));
        if (j.dv) dvt = stream_load(reinterpret_cast<const pic_v2d_a8*>(j.dv + o));
        s[d] = s[d] + (gx[0] * dxt[0] + gv[0] * dvt[0]);
        s[d] = s[d] + (gx[1] * dxt[1] + gv[1] * dvt[1]);
      }
    } else {
      double gx, gv;
      phase_gather(x[row + i], v[row + i], gr, a, cx, cv, gx, gv);
#pragma unroll
      for (int d = 0; d < KD; ++d) {
        if (d >= j.K) break;
        const size_t o = (size_t)d * j.dstride + drow + i;
        const double dx = j.dx ? j.dx[o] : 0.0, dv = j.dv ? j.dv[o] : 0.0;
        s[d] = s[d] + (gx * dx + gv * dv);
      }
    }
  }
#pragma unroll
  for (int d = 0; d < KD; ++d) {
    if (d >= j.K) break;
    const double S = block_sum<WAVES>(s[d], ws);
    if (threadIdx.x == 0) j.part[((size_t)d * j.num_envs + env) * j.chunks + blockIdx.x] = S;
  }
}

// One single-lane workgroup per (environment, direction): the chunks' sums in ascending order into out[d * out_dstride + env].
__global__ __launch_bounds__(1) void phase_jvp_finish_kernel(const double* __restrict__ part, int chunks, int num_envs,
                                                             double* __restrict__ out, long long out_dstride) {
  const int env = blockIdx.x, d = blockIdx.y;
  const double* p = part + ((size_t)d * num_envs + env) * chunks;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += p[c];
  out[(size_t)d * out_dstride + env] = s;
}

}  // namespace
