// pic_record.h -- the rollout recorder's two kernels (include/picstep.h: pic_record_*): a particle pass that
// builds the marginal and phase-space histograms of every environment, and a per-environment finishing kernel for the mesh
// reductions.  Off the step path: they run after a recorded step and read what it left.
#pragma once
#include "pic_aux.h"

namespace {

// the particle pass (host_blocks.h: record_plan sizes its grid and lays out its LDS): x_hist | v_hist | inside of record slot `rec` (zeroed at pic_record_start) and the phase counts
// ([env][px][pv] scratch, zeroed by the finishing kernel of the previous record)
struct RecordHistArgs {
  unsigned* rec;          // [env][u_stride]: x_hist [xb], v_hist [vb], inside [1]
  long long u_stride;
  unsigned* phase;        // [env][px * pv], or null
  int xb, vb, px, pv;
  int phase_lds;          // 1: the phase histogram has an LDS copy per workgroup; 0: global atomics
  int rr;                 // copies of each marginal bin in LDS (a power of two): lane l adds to copy l % rr
  long long N, ld;
  long long tiles_per_wg; // 16-byte tiles (VEC particles) per workgroup and lane column: a workgroup's range is contiguous
  double L, vmin, vmax;
  double sx, sv, spx, spv; // np.linspace steps of the four edge sets
};

// One read of x and v, 16 bytes per lane as the sweeps load them; every bin add goes to an LDS sub-histogram (ds_add_u32) and a
// workgroup flushes one global atomic per non-zero bin.  Counts are integers: the result does not depend on the grid.
// A velocity distribution puts most particles of a wave into a few bins: the marginals keep rr copies of every bin in consecutive
// words (copy l % rr for lane l, so lanes of one hot bin hit different banks), and the phase histogram's rows are padded to pv + 1
// words (its bank follows ix as well as iv).
template <typename P>
__global__ __launch_bounds__(BLOCK) void record_hist_kernel(const typename P::X* __restrict__ x,
                                                            const typename P::V* __restrict__ v, RecordHistArgs a) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int rr = a.rr, lane_copy = threadIdx.x & (a.rr - 1);
  unsigned* hx = reinterpret_cast<unsigned*>(smem_raw);           // [xb][rr]
  unsigned* hv = hx + (size_t)a.xb * rr;                           // [vb][rr]
  unsigned* hin = hv + (size_t)a.vb * rr;                          // [1]
  unsigned* hp = hin + 1;                                          // [px][pv + 1] when phase_lds
  const int env = blockIdx.y;
  const int nb2 = a.px * a.pv, prow = a.pv + 1;
  const int lds_words = (a.xb + a.vb) * rr + 1 + (a.phase_lds ? a.px * prow : 0);
  for (int i = threadIdx.x; i < lds_words; i += BLOCK) hx[i] = 0u;
  __syncthreads();
  unsigned* gp = a.phase ? a.phase + (size_t)env * nb2 : nullptr;
  const typename P::XV* xv = reinterpret_cast<const typename P::XV*>(x + (size_t)env * a.ld);
  const typename P::VV* vv = reinterpret_cast<const typename P::VV*>(v + (size_t)env * a.ld);
  const long long ntiles = (a.N + P::VEC - 1) / P::VEC;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_wg * BLOCK;
  long long t1 = t0 + a.tiles_per_wg * BLOCK;
  t1 = t1 < ntiles ? t1 : ntiles;
  unsigned inside = 0;
  for (long long t = t0 + threadIdx.x; t < t1; t += BLOCK) {
    const typename P::XV xt = stream_load(xv + t);
    const typename P::VV vt = stream_load(vv + t);
#pragma unroll
    for (int k = 0; k < P::VEC; ++k) {
      if (t * P::VEC + k >= a.N) break;
      const double xs = pos_to_length<P>(xt[k], a.L), vs = (double)vt[k];
      inside += (xs >= 0.0 && xs <= a.L && vs >= a.vmin && vs <= a.vmax) ? 1u : 0u;
      if (a.xb) {
        const int b = hist_bin(xs, 0.0, a.L, a.sx, a.xb);
        if (b >= 0) atomicAdd(&hx[b * rr + lane_copy], 1u);
      }
      if (a.vb) {
        const int b = hist_bin(vs, a.vmin, a.vmax, a.sv, a.vb);
        if (b >= 0) atomicAdd(&hv[b * rr + lane_copy], 1u);
      }
      if (nb2) {
        const int ix = hist_bin(xs, 0.0, a.L, a.spx, a.px);
        const int iv = hist_bin(vs, a.vmin, a.vmax, a.spv, a.pv);
        if (ix >= 0 && iv >= 0) {
          if (a.phase_lds) atomicAdd(&hp[ix * prow + iv], 1u);
          else atomicAdd(&gp[(size_t)ix * a.pv + iv], 1u);
        }
      }
    }
  }
  if (inside) atomicAdd(hin, inside);
  __syncthreads();
  unsigned* r = a.rec + (size_t)env * a.u_stride;
  for (int i = threadIdx.x; i < a.xb + a.vb; i += BLOCK) {
    unsigned c = 0;
    for (int k = 0; k < rr; ++k) c += hx[i * rr + k];
    if (c) atomicAdd(&r[i], c);
  }
  if (threadIdx.x == 0 && *hin) atomicAdd(&r[a.xb + a.vb], *hin);
  if (a.phase_lds)
    for (int i = threadIdx.x; i < nb2; i += BLOCK) {
      const unsigned c = hp[(i / a.pv) * prow + i % a.pv];
      if (c) atomicAdd(&gp[i], c);
    }
}

struct RecordFinishArgs {
  const double* E_mesh;
  const double* KE;          // KE | PE | PE_reward, [3][env]
  const double* tw;          // twiddles of modes 1..tw_rows (twiddle_kernel)
  int tw_rows, Ng, M;
  double dx;
  double* rec;               // [env][d_stride]: KE, PE, PE_reward, field_energy, entropy, kl, re [M], im [M]
  long long d_stride;
  unsigned* phase;           // [env][nb2] counts of this record (cleared here behind the read), or null
  int nb2;
  const double* feq;         // [nb2] or null
  double norm, dxdv;         // f = counts * norm; entropy and KL are sums times dxdv
};

// One workgroup per environment; every reduction in a fixed order (the threads' strided partial sums, then block_sum's).
__global__ __launch_bounds__(BLOCK) void record_finish_kernel(RecordFinishArgs a) {
  __shared__ double ws[2 * WAVES];
  const int env = blockIdx.x;
  const double* E = a.E_mesh + (size_t)env * a.Ng;
  double* r = a.rec + (size_t)env * a.d_stride;
  double e2 = 0.0, e0 = 0.0;
  for (int j = threadIdx.x; j < a.Ng; j += BLOCK) {
    const double e = E[j];
    e2 += e * e;
    e0 += e;
  }
  double s2, s0;
  block_sum2<WAVES>(e2, e0, ws, s2, s0);
  if (threadIdx.x == 0) {
    r[0] = a.KE[env];
    r[1] = a.KE[gridDim.x + env];
    r[2] = a.KE[2 * (size_t)gridDim.x + env];
    r[3] = s2 * a.dx;
    if (a.M > 0) {               // row 0: the mean (twiddles 1, 0)
      r[6] = s0 / a.Ng * 2.0;
      r[6 + a.M] = 0.0;
    }
  }
  for (int m = 1; m < a.M; ++m) {
    double re, im;
    mesh_mode<WAVES>(E, a.tw + (size_t)(m - 1) * a.Ng, a.tw + ((size_t)a.tw_rows + m - 1) * a.Ng, a.Ng, ws, re, im);
    if (threadIdx.x == 0) {
      r[6 + m] = re;
      r[6 + a.M + m] = im;
    }
  }
  if (a.nb2 > 0) {
    unsigned* c = a.phase + (size_t)env * a.nb2;
    double s = 0.0, k = 0.0;
    for (int i = threadIdx.x; i < a.nb2; i += BLOCK) {
      const double f = (double)c[i] * a.norm;
      c[i] = 0u;
      if (f > 0.0) {
        s += f * log(f);
        if (a.feq) k += f * log(f / (a.feq[i] + 1e-12));
      }
    }
    double S, K;
    block_sum2<WAVES>(s, k, ws, S, K);
    if (threadIdx.x == 0) {
      r[4] = -S * a.dxdv;
      r[5] = a.feq ? K * a.dxdv : __builtin_nan("");
    }
  } else if (threadIdx.x == 0) {
    r[4] = __builtin_nan("");
    r[5] = __builtin_nan("");
  }
}

}  // namespace
