// pic_adjoint.h -- the reverse pass of a taped rollout (pic_tape_*): the vector-Jacobian product of T Yoshida-4
// steps (float64 particles, float64 positions, 64-bit fixed-point deposits, CIC) with respect to every step's external field and
// the initial particles.  Kernels off the step path; none of the forward's kernels is changed.
//
//   tape_ext_kernel        the external field e_t of each step of a call, as the forward builds it (mesh, or actuator product)
//   adjoint_replay_kernel  step t again from its (x_t, v_t) with the forward's helpers in the forward's order: deposit of q_K
//                          (K = 1..3), or of x' with x', v' stored (K = 4); the fields between them are field_solve_kernel's
//   tape_compare_kernel    replayed end of a segment against the state the forward left there (must be equal bit for bit)
//   adjoint_pass_kernel    one sub-stage of the reverse step: lambda through the gather, kick and drift (K = 3, 2, 1; K = 0
//                          closes the step through the first drift)
//   adjoint_deposit_kernel the adjoint deposit mu_K = sum_i (-d_K dt lambda_p,i) W(q_K,i) in 64-bit fixed point
//   adjoint_mesh_kernel    mu (or the refresh cotangent) -> nu = K^T m = -K (m - mean m), and e-bar_t += mu
//   adjoint_actions_kernel the actuator part: a-bar_t = B^T e-bar_t
//   law_adjoint_kernel     a step of the gain law a = G m(E): E-bar = J^T (G^T a-bar + m-bar), a cotangent on the
//                          field the step started from, which the refresh of the step before adds to its m; without a gain
//                          E-bar = J^T m-bar alone (a walk's cotangent on an observation of M_o modes)
//   adjoint_start_kernel   lambda_x0 += s W'(x_0) . nu: the field at the start of the tape, read by a first law step; plus
//                          the caller's cotangents on the starting state (pic_tape_walk_end)
#pragma once
#include "pic_device.h"
#include "pic_solve.h"

namespace {

constexpr int ABLOCK = 256;
constexpr int AWAVES = ABLOCK / 64;

struct AdjArgs {
  long long N, ld;
  int Ng;
  int fg;              // fractional bits of the forward's deposits (the replay makes the same integer sums)
  int bitsN;           // 2^bitsN >= N: headroom of the adjoint deposits' unit
  int pad_;
  double magic;        // the forward's fixed-point magic (pic_device.h: to_fixed)
  double L, dx, dt, scale, N_over_L;
  double c[4], d[4];   // Yoshida-4 drift / kick coefficients, d[0] unused
};

// x_t, v_t of a step and its three sub-stage fields [3][env][Ng] (external field included)
struct AdjStep {
  const double* x;
  const double* v;
  const double* F;
  long long fstride;   // elements from one sub-stage field to the next (num_envs * Ng)
};

// Cell and CIC weights of q exactly as the forward's locate: wrap, then locate_in_box.  jr: the right node.
__device__ __forceinline__ void adj_locate(double q, const Consts<PosF64>& k, double& xw, int& j, int& jr, double (&w)[3],
                                           unsigned& bad) {
  unsigned frac;
  locate<PosF64, PIC_CIC>(q, k, xw, j, w, frac, bad);
  jr = j + 1 == k.Ng ? 0 : j + 1;
}

// W'(q) . mesh: the weight slopes are -1/dx (left node) and +1/dx (right node)
__device__ __forceinline__ double slope_dot(const double* __restrict__ m, int j, int jr, double dx) {
  return (m[jr] - m[j]) / dx;
}

// Positions q_1..q_{upto} and momenta p_1..p_{min(upto, 3)} of one particle of step t, recomputed from (x, v) and the step's
// fields with push_one's operations in push_one's order (PosF64): the same bits as the forward.  q[0] is unused; p[0] = v.
template <int UPTO>
__device__ __forceinline__ void replay_particle(double x, double v, const AdjStep& s, size_t row, const Consts<PosF64>& k,
                                                const AdjArgs& a, double (&q)[5], double (&p)[4], unsigned& bad) {
  p[0] = v;
  q[1] = x + (a.c[0] * v) * a.dt;                                 // integration.py:42, c1
#pragma unroll
  for (int m = 1; m < UPTO && m <= 3; ++m) {
    double w[3], xw;
    int j, jr;
    adj_locate(q[m], k, xw, j, jr, w, bad);
    const double* F = s.F + (size_t)(m - 1) * s.fstride + row;
    const double E = w[0] * F[j] + w[1] * F[jr];                  // gather_field<double, CIC> (Es[Ng] is node 0)
    p[m] = p[m - 1] + (a.d[m] * (-E)) * a.dt;                     // integration.py:32
    q[m + 1] = q[m] + (a.c[m] * p[m]) * a.dt;                     // integration.py:42
  }
}

// LDS mesh of a workgroup (Ng + 1 slots: the right node of the last cell is slot Ng) -> the environment's global row
__device__ __forceinline__ void adj_flush(const unsigned long long* __restrict__ lds, int Ng, acc_t* __restrict__ row) {
  unsigned long long* out = reinterpret_cast<unsigned long long*>(row);
  for (int c = threadIdx.x; c < Ng; c += ABLOCK) {
    unsigned long long t = lds[c];
    if (c == 0) t += lds[Ng];
    if (t) atomicAdd(out + c, t);
  }
}

// K = 1..3: deposit q_K into acc [env][Ng] (the forward's fixed-point weights); K = 4: deposit x' = wrap(q_4) and store x', v'
template <int K>
__global__ __launch_bounds__(ABLOCK) void adjoint_replay_kernel(AdjStep s, acc_t* __restrict__ acc, double* __restrict__ xo,
                                                                double* __restrict__ vo, AdjArgs a, unsigned long long* bad_out) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.y, Ng = a.Ng;
  for (int c = threadIdx.x; c <= Ng; c += ABLOCK) lds[c] = 0ull;
  __syncthreads();
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  unsigned bad = 0u;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    double q[5], p[4];
    replay_particle<K>(s.x[prow + i], s.v[prow + i], s, row, k, a, q, p, bad);
    double w[3], xw;
    int j, jr;
    adj_locate(q[K], k, xw, j, jr, w, bad);
    atomicAdd(lds + j, (unsigned long long)to_fixed(w[0], a.magic));
    atomicAdd(lds + j + 1, (unsigned long long)to_fixed(w[1], a.magic));
    if (K == 4) {
      xo[prow + i] = xw;                                          // pic.py:139 (+ util.py:51)
      vo[prow + i] = p[3];
    }
  }
  __syncthreads();
  adj_flush(lds, Ng, acc + row);
  if (bad) atomicAdd(bad_out, (unsigned long long)bad);
}

// bit-for-bit comparison of the first N elements of every row of two [env][ld] arrays (x and v at once)
__global__ __launch_bounds__(ABLOCK) void tape_compare_kernel(const double* __restrict__ x0, const double* __restrict__ v0,
                                                              const double* __restrict__ x1, const double* __restrict__ v1,
                                                              long long N, long long ld, unsigned long long* __restrict__ count) {
  const size_t prow = (size_t)blockIdx.y * ld;
  unsigned long long n = 0;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * ABLOCK) {
    n += __double_as_longlong(x0[prow + i]) != __double_as_longlong(x1[prow + i]);
    n += __double_as_longlong(v0[prow + i]) != __double_as_longlong(v1[prow + i]);
  }
  if (n) atomicAdd(count, n);
}

// the kick coefficient of sub-stage K: d_K (-E) dt differentiated by E, times lambda_p
__device__ __forceinline__ double kick_coef(const AdjArgs& a, int K, double lp) { return (-a.d[K] * a.dt) * lp; }

// per-environment max |c| of a pass, as the bit pattern of a non-negative double (ordered like the value): order-independent
__device__ __forceinline__ void block_max_to(double v, unsigned long long* __restrict__ out) {
  unsigned long long b = (unsigned long long)__double_as_longlong(fabs(v));
  if (!(fabs(v) <= 1.7976931348623157e308)) b = 0x7FF0000000000000ull;        // inf / NaN: saturate (the unit is then 2^1024)
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(b, off);
    b = o > b ? o : b;
  }
  if ((threadIdx.x & 63) == 0 && b) atomicMax(out, b);
}

// One sub-stage of the reverse step t.  lx, lv [env][ld]: lambda_q, lambda_p in and out.
//   K = 3: the refresh (lambda_x' += s W'(x') . nu, lambda_v' += a_KE v'), the last drift, then the kick of sub-stage 3 without
//          its deposit part: lambda_q3 = lambda_q4 + c W'(q3) . F3 with c = -d3 dt lambda_p3
//   K = 2, 1: lambda_q(K+1) += s W'(q(K+1)) . nu(K+1) (the deposit of the pass before), drift K+1, kick K as above
//   K = 0: lambda_q1 += s W'(q1) . nu1; lambda_x = lambda_q1, lambda_v = lambda_p1 + c1 dt lambda_q1
// nu: [env][Ng] or null (K = 3 without an energy cotangent on PE / PE_reward); cot: [3][env] of step t (K = 3), or null.
// cx, cv [env][cld] (K = 3, each optional): cotangents on the state step t left (a walk's injection), added to
// lambda_x', lambda_v' before the refresh terms.
template <int K>
__global__ __launch_bounds__(ABLOCK) void adjoint_pass_kernel(AdjStep s, const double* __restrict__ nu, const double* __restrict__ cot,
                                                              double* __restrict__ lx, double* __restrict__ lv,
                                                              unsigned long long* __restrict__ cmax, AdjArgs a, int num_envs,
                                                              const double* __restrict__ cx = nullptr,
                                                              const double* __restrict__ cv = nullptr, long long cld = 0) {
  const int env = blockIdx.y, Ng = a.Ng;
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  const double* nue = nu ? nu + row : nullptr;
  const double a_ke = (K == 3 && cot) ? cot[env] : 0.0;
  const size_t crow = (size_t)env * cld;
  unsigned bad = 0u;
  double cm = 0.0;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    double q[5], p[4];
    replay_particle<(K == 0 ? 1 : K + 1)>(s.x[prow + i], s.v[prow + i], s, row, k, a, q, p, bad);
    double lq = lx[prow + i], lp = lv[prow + i];
    double w[3], xw;
    int j, jr;
    if (K == 3) {
      if (cx) lq = lq + cx[crow + i];                              // lambda_x(t+1) += x-bar(t+1)
      if (cv) lp = lp + cv[crow + i];                              // lambda_v(t+1) += v-bar(t+1)
      adj_locate(q[4], k, xw, j, jr, w, bad);                      // x' = wrap(q4): the refresh deposit's cell
      if (nue) lq = lq + a.scale * slope_dot(nue, j, jr, a.dx);
      lp = lp + a_ke * p[3];                                       // KE = 0.5 sum v'^2
      lp = lp + a.c[3] * a.dt * lq;                                // q4 = q3 + c4 p3 dt
    } else {
      adj_locate(q[K + 1], k, xw, j, jr, w, bad);
      lq = lq + a.scale * slope_dot(nue, j, jr, a.dx);             // F_{K+1} depends on q_{K+1} through its deposit
      if (K > 0) lp = lp + a.c[K] * a.dt * lq;                     // q_{K+1} = q_K + c_{K+1} p_K dt
      else lp = lp + a.c[0] * a.dt * lq;                           // q1 = x + c1 v dt
    }
    if (K > 0) {
      adj_locate(q[K], k, xw, j, jr, w, bad);
      const double c = kick_coef(a, K, lp);
      lq = lq + c * slope_dot(s.F + (size_t)(K - 1) * s.fstride + row, j, jr, a.dx);
      cm = fmax(cm, fabs(c));
      if (!(fabs(c) <= 1.7976931348623157e308)) cm = c;            // keep a non-finite value visible to the max
    }
    lx[prow + i] = lq;
    lv[prow + i] = lp;
  }
  if (K > 0) block_max_to(cm, cmax + env);
  (void)bad;
  (void)num_envs;
}

// exponent of the unit of an environment's adjoint deposit: every |c w| <= max|c| < 2^e, N of them sum below 2^(e + bitsN), and
// the unit 2^(e + bitsN - 61) keeps that below 2^61 units (two bits of headroom in an int64: no overflow, whatever the data)
__device__ __forceinline__ int adj_unit_exp(unsigned long long maxbits, int bitsN) {
  const double m = __longlong_as_double((long long)maxbits);
  if (!(m > 0.0)) return 0;
  if (!(m <= 1.7976931348623157e308)) return 1024 + bitsN - 61;
  return ilogb(m) + 1 + bitsN - 61;
}

// mu_K [env][Ng] += round(c W(q_K) / unit) for every particle, c = -d_K dt lambda_p (lv after pass K)
template <int K>
__global__ __launch_bounds__(ABLOCK) void adjoint_deposit_kernel(AdjStep s, const double* __restrict__ lv,
                                                                 const unsigned long long* __restrict__ cmax, acc_t* __restrict__ acc,
                                                                 AdjArgs a) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem_raw);
  const int env = blockIdx.y, Ng = a.Ng;
  const unsigned long long mb = cmax[env];
  if (mb == 0ull) return;                                          // every coefficient is zero: mu is zero
  for (int c = threadIdx.x; c <= Ng; c += ABLOCK) lds[c] = 0ull;
  __syncthreads();
  const int ue = adj_unit_exp(mb, a.bitsN);
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  unsigned bad = 0u;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    double q[5], p[4];
    replay_particle<K>(s.x[prow + i], s.v[prow + i], s, row, k, a, q, p, bad);
    double w[3], xw;
    int j, jr;
    adj_locate(q[K], k, xw, j, jr, w, bad);
    const double c = kick_coef(a, K, lv[prow + i]);
    atomicAdd(lds + j, (unsigned long long)__double2ll_rn(ldexp(c * w[0], -ue)));
    atomicAdd(lds + j + 1, (unsigned long long)__double2ll_rn(ldexp(c * w[1], -ue)));
  }
  __syncthreads();
  adj_flush(lds, Ng, acc + row);
}

// One workgroup per environment.  Deposit mode (acc != null): m = mu = acc * unit (the row is cleared behind the read, and the
// environment's max with it), e-bar_t += mu.  Refresh mode (acc == null): m = (a_PE N/L + a_PEr) dx M for the post-step field M
// and the cotangents of step t, cot [3][env] (M null: m = 0), plus `add` [env][Ng] if given (the E-bar of a gain-law step that
// reads this field).  Either way nu = K^T m = -K (m - mean m) (the field operator is antisymmetric: the central difference is,
// the periodic Poisson inverse is symmetric, and both are circulant), through the forward's scans.
__global__ __launch_bounds__(SBLOCK) void adjoint_mesh_kernel(acc_t* __restrict__ acc, unsigned long long* __restrict__ cmax,
                                                              const double* __restrict__ M, const double* __restrict__ cot,
                                                              double* __restrict__ gext, double* __restrict__ nu, AdjArgs a,
                                                              int num_envs, const double* __restrict__ add) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  double* sb = reinterpret_cast<double*>(smem_raw);
  __shared__ double ws[2 * SWAVES];
  __shared__ double slot[2];
  const int env = blockIdx.x, Ng = a.Ng, tid = threadIdx.x;
  const size_t row = (size_t)env * Ng;
  double loc = 0.0;
  if (acc) {
    const unsigned long long mb = cmax[env];
    const double unit = ldexp(1.0, adj_unit_exp(mb, a.bitsN));
    for (int j = tid; j < Ng; j += SBLOCK) {
      const double mu = mb ? (double)acc[row + j] * unit : 0.0;
      acc[row + j] = 0;
      gext[row + j] += mu;
      sb[j] = mu;
      loc += mu;
    }
  } else {
    const double f = M ? (cot[(size_t)num_envs + env] * a.N_over_L + cot[2 * (size_t)num_envs + env]) * a.dx : 0.0;
    for (int j = tid; j < Ng; j += SBLOCK) {
      double m = M ? f * M[row + j] : 0.0;
      if (add) m = m + add[row + j];
      sb[j] = m;
      loc += m;
    }
  }
  const double mean = block_sum<SWAVES>(loc, ws) / (double)Ng;      // (ends with a barrier: every cmax read is done)
  if (acc && tid == 0) cmax[env] = 0ull;
  for (int j = tid; j < Ng; j += SBLOCK) sb[j] = -(sb[j] - mean);
  __syncthreads();
  scan_fields(sb, nullptr, Ng, a.dx, slot);
  __syncthreads();
  const double gmean = slot[0];
  for (int j = tid; j < Ng; j += SBLOCK) {
    const double gp = sb[j] - gmean;
    const double gm = sb[j == 0 ? Ng - 1 : j - 1] - gmean;
    nu[row + j] = -0.5 * (gp + gm);
  }
}

// e_t [step][env][Ng] of the n steps of a call: grid (num_envs, n).  The actuator's field is actuator_field, the function every
// forward path builds it with (same doubles); a held action given on the host travels in the argument block (act_inline).
struct TapeExtArgs {
  const double* ext;        // [env][Ng] of the call's first step, or null
  const double* act;        // [env][2M] of the call's first step, or null (act_inline: ignored)
  const double* basis;      // [2][Ng][M]
  double* out;              // e of the call's first step
  long long ext_step, act_step;
  int Ng, M, num_envs, act_inline;
};

__global__ __launch_bounds__(ABLOCK) void tape_ext_kernel(TapeExtArgs t, InlineDoubles act_inline) {
  (void)act_inline;
  const int env = blockIdx.x, s = blockIdx.y, Ng = t.Ng;
  double* out = t.out + ((size_t)s * t.num_envs + env) * Ng;
  const double* act = t.act_inline ? kernarg_ptr<double>(sizeof(TapeExtArgs)) : t.act;
  if (act) act += (size_t)s * t.act_step + (size_t)env * 2 * t.M;
  const double* ext = t.ext ? t.ext + (size_t)s * t.ext_step + (size_t)env * Ng : nullptr;
  for (int j = threadIdx.x; j < Ng; j += ABLOCK)
    out[j] = act ? actuator_field(t.basis, t.basis + (size_t)Ng * t.M, act, j, t.M) : (ext ? ext[j] : 0.0);
}
static_assert(sizeof(TapeExtArgs) % 8 == 0, "the inline actions follow the arguments");

// a-bar [T][env][2M] = B^T e-bar (actuator.py:54-63 transposed): grid (num_envs, T), one thread per coefficient
__global__ __launch_bounds__(ABLOCK) void adjoint_actions_kernel(const double* __restrict__ gext, const double* __restrict__ basis,
                                                                 double* __restrict__ gact, int Ng, int M, int num_envs) {
  const int env = blockIdx.x, t = blockIdx.y;
  const double* g = gext + ((size_t)t * num_envs + env) * Ng;
  for (int m = threadIdx.x; m < 2 * M; m += ABLOCK) {
    const double* b = basis + (m < M ? 0 : (size_t)Ng * M);
    const int mm = m < M ? m : m - M;
    double s = 0.0;
    for (int j = 0; j < Ng; ++j) s += b[(size_t)j * M + mm] * g[j];
    gact[((size_t)t * num_envs + env) * 2 * M + m] = s;
  }
}

// E-bar [env][Ng] of the field E a step started from, read through its modes m = (Re E_1..Re E_R, Im E_1..Im E_R) (mesh_mode's
// map, spectrum.py:16).  A gain-law step (gain non-null, pic_device.h: feedback_action) reads M of them: a-bar = B^T e-bar (in
// another order than adjoint_actions_kernel's), m-bar_k = G^T a-bar + cot_m (ascending i).  cot_m [env][2 Mc] (or null): a
// cotangent on Mc modes (the law's own, or a walk's observation); without a gain m-bar = cot_m alone.  With
// R = max(M of the gain, Mc): E-bar_j = 2/Ng sum_m (m-bar_Re,m cos - m-bar_Im,m sin)(2 pi m j / Ng).  Grid (num_envs); dynamic
// LDS of 2 (Mg + R) doubles.
__global__ __launch_bounds__(ABLOCK) void law_adjoint_kernel(const double* __restrict__ gext, const double* __restrict__ basis,
                                                             const double* __restrict__ gain, const double* __restrict__ cot_m,
                                                             const double* __restrict__ tw, int rows, double* __restrict__ Ebar,
                                                             int Ng, int M, int Mc) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int Mg = gain ? M : 0, R = Mg > Mc ? Mg : Mc;
  double* sa = reinterpret_cast<double*>(smem_raw);
  double* sm = sa + 2 * Mg;
  const int env = blockIdx.x, n = 2 * Mg, tid = threadIdx.x, lane = tid & 63;
  const double* g = gext + (size_t)env * Ng;
  for (int m = tid >> 6; m < n; m += AWAVES) {                    // one wave per coefficient, a fixed-order wave sum
    const double* b = basis + (m < M ? 0 : (size_t)Ng * M);
    const int mm = m < M ? m : m - M;
    double s = 0.0;
    for (int j = lane; j < Ng; j += 64) s += b[(size_t)j * M + mm] * g[j];
    s = wave_sum(s);
    if (lane == 0) sa[m] = s;
  }
  __syncthreads();
  const double* G = gain ? gain + (size_t)env * n * n : nullptr;
  const double* cm = cot_m ? cot_m + (size_t)env * 2 * Mc : nullptr;
  for (int r = tid; r < 2 * R; r += ABLOCK) {
    const int m = r < R ? r : r - R, im = r < R ? 0 : 1;
    const double c = cm && m < Mc ? cm[im * Mc + m] : 0.0;
    double s;
    if (m < Mg) {
      const int k = im * Mg + m;
      s = 0.0;
      for (int i = 0; i < n; ++i) s += G[(size_t)i * n + k] * sa[i];
      s = s + c;
    } else {
      s = c;
    }
    sm[r] = s;
  }
  __syncthreads();
  const double c = 2.0 / Ng;
  for (int j = tid; j < Ng; j += ABLOCK) {
    double s = 0.0;
    for (int m = 0; m < R; ++m) {
      s += sm[m] * tw[(size_t)m * Ng + j];
      s -= sm[R + m] * tw[((size_t)rows + m) * Ng + j];
    }
    Ebar[(size_t)env * Ng + j] = c * s;
  }
}

// lambda_x += s W'(x) . nu at positions x [env][ld] (the tape's first checkpoint): the deposit of the field the tape started from
// (nu null: none); then lambda_x += cx, lambda_v += cv [env][cld] (each optional: a walk's cotangents on the starting state)
__global__ __launch_bounds__(ABLOCK) void adjoint_start_kernel(const double* __restrict__ x, const double* __restrict__ nu,
                                                               double* __restrict__ lx, AdjArgs a, double* __restrict__ lv = nullptr,
                                                               const double* __restrict__ cx = nullptr,
                                                               const double* __restrict__ cv = nullptr, long long cld = 0) {
  const int env = blockIdx.y, Ng = a.Ng;
  const Consts<PosF64> k(a.L, a.dx, Ng);
  const size_t prow = (size_t)env * a.ld, row = (size_t)env * Ng;
  unsigned bad = 0u;
  for (long long i = (long long)blockIdx.x * ABLOCK + threadIdx.x; i < a.N; i += (long long)gridDim.x * ABLOCK) {
    if (nu) {
      double w[3], xw;
      int j, jr;
      adj_locate(x[prow + i], k, xw, j, jr, w, bad);
      lx[prow + i] = lx[prow + i] + a.scale * slope_dot(nu + row, j, jr, a.dx);
    }
    if (cx) lx[prow + i] = lx[prow + i] + cx[(size_t)env * cld + i];
    if (cv) lv[prow + i] = lv[prow + i] + cv[(size_t)env * cld + i];
  }
  (void)bad;
}

}  // namespace
