// pic_tangent.h -- the forward-mode pass of a taped rollout (pic_tape_tangent): the Jacobian-vector product of T
// Yoshida-4 steps in K <= 8 directions at once, on the states, sub-stage fields and post-step fields that walk_replay rebuilds
// (pic_adjoint.h).  Kernels off the step path; none of the forward's or the adjoint's kernels is changed.
//
//   tangent_start_kernel   max |dq_1| = max |dx + c1 dt dv| per direction and environment: the unit of the first deposit
//   tangent_deposit_kernel the deposit of a direction, drho_j = s sum_i W'_j(q_S,i) dq_S,i, in 64-bit fixed point (S = 1..3:
//                          the sub-stage positions; S = 4: x' = wrap(q_4), plus the integer sum behind dKE = sum p_3 dp_3)
//   tangent_mesh_kernel    drho -> dF = K drho + de_t (S = 1..3), or dM = K drho with dPE, dPE_reward, dKE (S = 4)
//   tangent_pass_kernel    sub-stage S of every direction: dE_S through the gather, the kick and the drift; the maxima behind
//                          the next deposit's unit
//
// The closed loop in forward mode (pic_tape_tangent_walk_*, pic_tape_tangent_feedback):
//   tangent_x_max_kernel          max |dx_0| per direction and environment: the unit of the deposit at the tape's start
//   tangent_start_deposit_kernel  drho(x_0; dx_0) at the stored starting positions (the forward twin of adjoint_start_kernel)
//   tangent_law_kernel            dm = J dM of the field tangent a step left (the observation's and the law's modes), and the next
//                                 law step's da = G dm + dG m
//   tangent_action_kernel         the caller's injection into a step's da row
//
// Every particle's base quantities (q_S, p_S, cell, weights, slope of F_S) come from replay_particle once per pass and serve all
// directions.  The tangent state is (dq, dp) [K][2][env][ld]: (dx, dv) at the start of a step, (dq_{S+1}, dp_S) after pass S.
#pragma once
#include "pic_adjoint.h"

namespace {

constexpr int kMaxTangents = 8;

// the tangent's working memory and geometry (views into the tape's tangent block)
struct TanArgs {
  double* st;                 // [K][2][env][ld] dq, dp
  long long dstride;          // elements from one direction's state to the next (2 env ld)
  long long vofs;             // from dq to dp (env ld)
  double* dF;                 // [K][env][Ng] the field tangent the next pass reads
  acc_t* acc;                 // [K][env][Ng] deposits, zero between uses
  acc_t* ke;                  // [K][env] integer sum behind dKE, zero between uses
  unsigned long long* umax;   // [3][K][env] max bit patterns, zero between uses: 0 the next deposit's |dq| (S = 2..4), 1 |p_3 dp_3|,
                              // 2 |dq_1| of the next step's first deposit
  int K, num_envs;
};

__device__ __forceinline__ unsigned long long* tan_max(const TanArgs& t, int slot, int d, int env) {
  return t.umax + ((size_t)slot * t.K + d) * t.num_envs + env;
}

// running max |v| whose non-finite values stay visible to block_max_to (which saturates them)
__device__ __forceinline__ void max_abs(double& m, double v) {
  m = fmax(m, fabs(v));
  if (!(fabs(v) <= 1.7976931348623157e308)) m = v;
}

// dq_1 = dx + (c1 dt) dv
__device__ __forceinline__ double tan_q1(const AdjArgs& a, double dx, double dv) { return dx + (a.c[0] * a.dt) * dv; }

// slot 2 <- max |dq_1| of the tangent state (grid (gx, env); directions one after the other)
__global__ __launch_bounds__(ABLOCK) void tangent_start_kernel(TanArgs t, AdjArgs a) {
  const int env = blockIdx.y;
  const size_t prow = (size_t)env * a.ld;
  for (int d = 0; d < t.K; ++d) {
    const double* sq = t.st + (size_t)d * t.dstride + prow;
    double m = 0.0;
    for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK)
      max_abs(m, tan_q1(a, sq[i], sq[t.vofs + i]));
    block_max_to(m, tan_max(t, 2, d, env));
  }
}

// sum over the 64 lanes of an integer (order-free), in every lane
__device__ __forceinline__ long long wave_isum(long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Deposits of directions d0 .. d0 + nd - 1 (grid (gx, env, groups of kd <= KB); LDS [kd][Ng + 1]): each particle adds -r to its left node
// and +r to its right node, r = round(dq / unit), unit = 2^(e + bitsN - 61) with max |dq| < 2^e (adj_unit_exp): the two halves
// cancel exactly, so sum drho = 0 in integers, and N particles stay below 2^61 units.  S = 4 also sums round(p_3 dp_3 / unit')
// per lane, then per wave, into ke (integer adds: order-free).
template <int S, int KB>
__global__ __launch_bounds__(ABLOCK) void tangent_deposit_kernel(AdjStep s, TanArgs t, AdjArgs a, int kd) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.y, Ng = a.Ng, d0 = blockIdx.z * kd;
  const int nd = min(kd, t.K - d0);
  for (int c = threadIdx.x; c < nd * (Ng + 1); c += ABLOCK) lds[c] = 0ull;
  int ue[KB], uk[KB];
  bool on[KB], onk[KB];
#pragma unroll
  for (int d = 0; d < KB; ++d) {
    const unsigned long long mb = d < nd ? *tan_max(t, S == 1 ? 2 : 0, d0 + d, env) : 0ull;
    on[d] = mb != 0ull;
    ue[d] = adj_unit_exp(mb, a.bitsN);
    const unsigned long long kb = (S == 4 && d < nd) ? *tan_max(t, 1, d0 + d, env) : 0ull;
    onk[d] = kb != 0ull;
    uk[d] = adj_unit_exp(kb, a.bitsN);
  }
  __syncthreads();
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  unsigned bad = 0u;
  long long kr[KB];
#pragma unroll
  for (int d = 0; d < KB; ++d) kr[d] = 0;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    double q[5], p[4];
    replay_particle<S>(s.x[prow + i], s.v[prow + i], s, row, k, a, q, p, bad);
    double w[3], xw;
    int j, jr;
    adj_locate(q[S], k, xw, j, jr, w, bad);
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      if (d >= nd) break;
      const double* sq = t.st + (size_t)(d0 + d) * t.dstride + prow + i;
      const double dq = S == 1 ? tan_q1(a, sq[0], sq[t.vofs]) : sq[0];
      if (on[d]) {
        const long long r = __double2ll_rn(ldexp(dq, -ue[d]));
        atomicAdd(lds + d * (Ng + 1) + j, (unsigned long long)(-r));
        atomicAdd(lds + d * (Ng + 1) + j + 1, (unsigned long long)r);
      }
      if (S == 4 && onk[d]) kr[d] += __double2ll_rn(ldexp(p[3] * sq[t.vofs], -uk[d]));
    }
  }
  __syncthreads();
  for (int d = 0; d < nd; ++d) adj_flush(lds + d * (Ng + 1), Ng, t.acc + (size_t)(d0 + d) * t.num_envs * Ng + row);
  if (S == 4) {
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      if (d >= nd) break;
      const long long v = wave_isum(kr[d]);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(t.ke + (size_t)(d0 + d) * t.num_envs + env),
                                                  (unsigned long long)v);
    }
  }
  (void)bad;
}

// what a mesh pass reads and writes besides the working memory
struct TanMeshIO {
  const double* ext;      // de_t [K][T][env][Ng] at step t of direction 0, or null
  const double* act;      // da_t [K][T][env][2M] at step t of direction 0, or null (through the actuator basis)
  const double* basis;    // [2][Ng][M]
  long long in_dstride;   // elements from one direction's input to the next (T env Ng, or T env 2M)
  const double* M;        // [env][Ng] post-step field of the step (S = 4)
  double* hist;           // [K][T][3][env] at step t of direction 0 (S = 4), or null
  double* Emesh;          // [K][T][env][Ng] at step t of direction 0 (S = 4), or null
  long long out_hstride, out_mstride;   // elements from one direction's hist / Emesh to the next
  int Mact;               // the actuator's modes
};

// One workgroup per (environment, direction): drho = acc unit s / dx (the row and the words it used cleared behind the read),
// b = drho - mean(drho), then K b through the forward's scans: dF_j = -(G_{j+1/2} + G_{j-1/2}) / 2 (+ de_t for S < 4).  S = 4:
// dPE_reward = dx sum_j M_j dM_j in a fixed-order workgroup sum, dPE = N/L dPE_reward, dKE = ke unit'.
template <int S>
__global__ __launch_bounds__(SBLOCK) void tangent_mesh_kernel(TanArgs t, TanMeshIO io, AdjArgs a) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* sb = reinterpret_cast<double*>(smem_raw);
  __shared__ double ws[2 * SWAVES];
  __shared__ double slot[2];
  const int env = blockIdx.x, d = blockIdx.y, Ng = a.Ng, tid = threadIdx.x;
  const size_t row = (size_t)env * Ng, drow = (size_t)d * t.num_envs * Ng + row;
  unsigned long long* mw = tan_max(t, S == 1 ? 2 : 0, d, env);
  const unsigned long long mb = *mw;
  const double unit = ldexp(1.0, adj_unit_exp(mb, a.bitsN)), f = a.scale / a.dx;
  double loc = 0.0;
  for (int j = tid; j < Ng; j += SBLOCK) {
    const double r = mb ? ((double)t.acc[drow + j] * unit) * f : 0.0;
    t.acc[drow + j] = 0;
    sb[j] = r;
    loc += r;
  }
  const double mean = block_sum<SWAVES>(loc, ws) / (double)Ng;      // (ends with a barrier: the word's read is done)
  if (tid == 0) *mw = 0ull;
  for (int j = tid; j < Ng; j += SBLOCK) sb[j] = sb[j] - mean;
  __syncthreads();
  scan_fields(sb, nullptr, Ng, a.dx, slot);
  __syncthreads();
  const double gmean = slot[0];
  double e2 = 0.0;
  const double* ext = io.ext ? io.ext + (size_t)d * io.in_dstride + row : nullptr;
  const double* act = io.act ? io.act + (size_t)d * io.in_dstride + (size_t)env * 2 * io.Mact : nullptr;
  double* em = io.Emesh ? io.Emesh + (size_t)d * io.out_mstride + row : nullptr;
  for (int j = tid; j < Ng; j += SBLOCK) {
    const double gp = sb[j] - gmean;
    const double gm = sb[j == 0 ? Ng - 1 : j - 1] - gmean;
    const double dE = -0.5 * (gp + gm);
    if (S < 4) {
      const double de = act ? actuator_field(io.basis, io.basis + (size_t)Ng * io.Mact, act, j, io.Mact) : (ext ? ext[j] : 0.0);
      t.dF[drow + j] = dE + de;
    } else {
      if (em) em[j] = dE;
      e2 += io.M[row + j] * dE;
    }
  }
  if (S == 4) {
    const double s = block_sum<SWAVES>(e2, ws);
    if (tid == 0) {
      unsigned long long* kw = tan_max(t, 1, d, env);
      acc_t* kacc = t.ke + (size_t)d * t.num_envs + env;
      const unsigned long long kb = *kw;
      const double dke = kb ? (double)*kacc * ldexp(1.0, adj_unit_exp(kb, a.bitsN)) : 0.0;
      *kacc = 0;
      *kw = 0ull;
      if (io.hist) {
        double* h = io.hist + (size_t)d * io.out_hstride;
        const double per = a.dx * s;
        h[env] = dke;
        h[(size_t)t.num_envs + env] = a.N_over_L * per;
        h[2 * (size_t)t.num_envs + env] = per;
      }
    }
  }
}

// Sub-stage S = 1..3 of every direction (grid (gx, env)): with q_S, p_S of the replay, its cell and weights and the slope of F_S,
//   dE = W(q_S) . dF_S + dq_S (F_S[jr] - F_S[j]) / dx,  dp_S = dp_{S-1} - (d_S dt) dE,  dq_{S+1} = dq_S + (c_{S+1} dt) dp_S
// (S = 1 starts from dq_1 = dx + c1 dt dv, dp_0 = dv), and the maxima behind the next deposits' units: |dq_{S+1}| (slot 0);
// S = 3 also |p_3 dp_3| (slot 1) and the next step's |dq_1| = |dq_4 + c1 dt dp_3| (slot 2).
template <int S, int KB>
__global__ __launch_bounds__(ABLOCK) void tangent_pass_kernel(AdjStep s, TanArgs t, AdjArgs a) {
  const int env = blockIdx.y, Ng = a.Ng;
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  const double* F = s.F + (size_t)(S - 1) * s.fstride + row;
  unsigned bad = 0u;
  double mq[KB], mk[KB], m1[KB];
#pragma unroll
  for (int d = 0; d < KB; ++d) mq[d] = mk[d] = m1[d] = 0.0;
  const double kick = a.d[S] * a.dt, drift = a.c[S] * a.dt;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    double q[5], p[4];
    replay_particle<S + 1>(s.x[prow + i], s.v[prow + i], s, row, k, a, q, p, bad);
    double w[3], xw;
    int j, jr;
    adj_locate(q[S], k, xw, j, jr, w, bad);
    const double slope = slope_dot(F, j, jr, a.dx);
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      if (d >= t.K) break;
      double* sq = t.st + (size_t)d * t.dstride + prow + i;
      const double* dF = t.dF + (size_t)d * t.num_envs * Ng + row;
      double dq = sq[0], dp = sq[t.vofs];
      if (S == 1) dq = tan_q1(a, dq, dp);
      const double dE = (w[0] * dF[j] + w[1] * dF[jr]) + dq * slope;
      dp = dp - kick * dE;
      dq = dq + drift * dp;
      sq[0] = dq;
      sq[t.vofs] = dp;
      max_abs(mq[d], dq);
      if (S == 3) {
        max_abs(mk[d], p[3] * dp);
        max_abs(m1[d], tan_q1(a, dq, dp));
      }
    }
  }
#pragma unroll
  for (int d = 0; d < KB; ++d) {
    if (d >= t.K) break;
    block_max_to(mq[d], tan_max(t, 0, d, env));
    if (S == 3) {
      block_max_to(mk[d], tan_max(t, 1, d, env));
      block_max_to(m1[d], tan_max(t, 2, d, env));
    }
  }
  (void)bad;
}

// ---------------------------------------------------------------------------------------------
// The closed loop in forward mode
// ---------------------------------------------------------------------------------------------
// slot 0 <- max |dx| of the tangent state (grid (gx, env); directions one after the other): the unit of tangent_start_deposit_kernel
__global__ __launch_bounds__(ABLOCK) void tangent_x_max_kernel(TanArgs t, AdjArgs a) {
  const int env = blockIdx.y;
  const size_t prow = (size_t)env * a.ld;
  for (int d = 0; d < t.K; ++d) {
    const double* sq = t.st + (size_t)d * t.dstride + prow;
    double m = 0.0;
    for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) max_abs(m, sq[i]);
    block_max_to(m, tan_max(t, 0, d, env));
  }
}

// tangent_deposit_kernel at stored positions x [env][ld] (the tape's first checkpoint) with dq = dx_0: the deposit behind the
// tangent of the field the tape started from, dE_0 = K drho(x_0; dx_0).  Same grid, LDS and integer sums (unit of slot 0).
template <int KB>
__global__ __launch_bounds__(ABLOCK) void tangent_start_deposit_kernel(const double* __restrict__ x, TanArgs t, AdjArgs a, int kd) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.y, Ng = a.Ng, d0 = blockIdx.z * kd;
  const int nd = min(kd, t.K - d0);
  for (int c = threadIdx.x; c < nd * (Ng + 1); c += ABLOCK) lds[c] = 0ull;
  int ue[KB];
  bool on[KB];
#pragma unroll
  for (int d = 0; d < KB; ++d) {
    const unsigned long long mb = d < nd ? *tan_max(t, 0, d0 + d, env) : 0ull;
    on[d] = mb != 0ull;
    ue[d] = adj_unit_exp(mb, a.bitsN);
  }
  __syncthreads();
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  unsigned bad = 0u;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    double w[3], xw;
    int j, jr;
    adj_locate(x[prow + i], k, xw, j, jr, w, bad);
#pragma unroll
    for (int d = 0; d < KB; ++d) {
      if (d >= nd) break;
      if (!on[d]) continue;
      const long long r = __double2ll_rn(ldexp(t.st[(size_t)(d0 + d) * t.dstride + prow + i], -ue[d]));
      atomicAdd(lds + d * (Ng + 1) + j, (unsigned long long)(-r));
      atomicAdd(lds + d * (Ng + 1) + j + 1, (unsigned long long)r);
    }
  }
  __syncthreads();
  for (int d = 0; d < nd; ++d) adj_flush(lds + d * (Ng + 1), Ng, t.acc + (size_t)(d0 + d) * t.num_envs * Ng + row);
  (void)bad;
}

// what tangent_law_kernel reads and writes
struct TanLawArgs {
  const double* dM;       // [K][env][Ng] the field tangent the step left
  const double* tw;       // [2][rows][Ng] cos | sin twiddles, row m-1 = mode m
  double* obs;            // [K][env][2 Mo] the observation's tangent, or null
  double* dm;             // [K][env][2M] the law's dm, or null (M = 0)
  const double* gain;     // [env][2M][2M] G of the step that reads this field, or null: not a law step
  const double* dgain;    // [K][env][2M][2M] dG, or null
  const double* modes;    // [env][2M] m of that step (with dgain)
  double* da;             // [K][env][2M] that step's da = G dm + dG m (with gain)
  int rows, Ng, M, Mo, num_envs, pad_;
};

// One workgroup per (environment, direction).  dm = J dM for R = max(M, Mo) modes, mesh_mode's map: one wave per coefficient,
// lane l sums the nodes l + 64 k in ascending k, then a fixed-order wave sum.  The first Mo modes go to obs, the first M to dm;
// if the next step is a law step, da_i = sum_k G[i][k] dm_k (gain_row: the forward law's rule) + sum_k dG[i][k] m_k (ascending k).
__global__ __launch_bounds__(ABLOCK) void tangent_law_kernel(TanLawArgs l) {
  __shared__ double sm[2 * kMaxFeedbackModes];
  const int env = blockIdx.x, d = blockIdx.y, Ng = l.Ng, M = l.M, Mo = l.Mo, R = M > Mo ? M : Mo;
  const int lane = threadIdx.x & 63;
  const size_t de = (size_t)d * l.num_envs + env;
  const double* dM = l.dM + de * Ng;
  for (int r = threadIdx.x >> 6; r < 2 * R; r += AWAVES) {
    const int m = r < R ? r : r - R, im = r < R ? 0 : 1;
    const double* tw = l.tw + ((size_t)(im ? l.rows : 0) + m) * Ng;
    double s = 0.0;
    if (im) for (int j = lane; j < Ng; j += 64) s -= dM[j] * tw[j];
    else for (int j = lane; j < Ng; j += 64) s += dM[j] * tw[j];
    s = wave_sum(s) / Ng * 2.0;
    if (lane == 0) {
      if (m < Mo) l.obs[de * 2 * Mo + (size_t)im * Mo + m] = s;
      if (m < M) {
        l.dm[de * 2 * M + (size_t)im * M + m] = s;
        sm[im * M + m] = s;
      }
    }
  }
  if (!l.gain) return;
  __syncthreads();
  const int n = 2 * M, i = threadIdx.x;
  if (i >= n) return;
  double a = gain_row(l.gain + ((size_t)env * n + i) * n, sm, n);
  if (l.dgain) {
    const double* dG = l.dgain + (de * n + i) * n;
    const double* mv = l.modes + (size_t)env * n;
    double b = 0.0;
    for (int k = 0; k < n; ++k) b += dG[k] * mv[k];
    a = a + b;
  }
  l.da[de * n + i] = a;
}

// row d of da [K][n] takes the caller's injection inj + d stride: added to the law's da (add), or alone
__global__ __launch_bounds__(ABLOCK) void tangent_action_kernel(double* __restrict__ da, const double* __restrict__ inj,
                                                                long long stride, int n, int add) {
  const int d = blockIdx.y;
  const int i = blockIdx.x * ABLOCK + threadIdx.x;
  if (i >= n) return;
  const double v = inj[(size_t)d * stride + i];
  da[(size_t)d * n + i] = add ? da[(size_t)d * n + i] + v : v;
}

}  // namespace
