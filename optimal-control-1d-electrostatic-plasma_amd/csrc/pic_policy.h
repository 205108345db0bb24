// pic_policy.h -- the MLP policy a = pi(o) on the modes of the mesh field (pic_policy_eval, pic_step_policy), its VJP (7p) and its JVP (7q).
// Included by picstep.hip only, behind pic_device.h.
#pragma once

#include "pic_device.h"

namespace {

constexpr int kPolicyMaxWidth = 256;     // widest layer: one thread of the workgroup owns one output (BLOCK >= 256)
constexpr int kPolicyMaxLayers = 4;
constexpr int kPolicyMaxObsModes = 64;
static_assert(BLOCK >= kPolicyMaxWidth, "one thread per output of a layer");

// One policy evaluation for every environment.  Pointers are those of environment 0 (and of the step the launch is for).
struct PolicyArgs {
  const double* E_mesh;      // [env][Ng] the field the observation is taken from (obs == null)
  const double* tw;          // [2][rows][Ng] twiddles (twiddle_kernel), rows >= Mo
  const double* obs;         // [env][2 Mo] a given observation, or null: the modes of E_mesh
  const double* obs_scale;   // [2 Mo] or null
  const double* params;      // per layer W [out][in] row-major, then b [out]
  const double* noise;       // [env][nA] eps, or null
  const double* std;         // [nA], or null: 1
  double* obs_out;           // [env][2 Mo] the observation (unscaled), or null
  double* pre_out;           // [env][nA] u, or null
  double* act;               // [env][nA] a, where the step's force evaluations read it, or null
  double* act_out;           // [env][nA] a second copy in the caller's device memory, or null
  long long env_params;      // doubles from one environment's parameters to the next (0: shared)
  double action_scale;
  int rows, Ng, Mo, n_layers;
  int w0, w1, w2, w3, w4;    // widths (scalars: an indexed member of the argument block would go through scratch)
  int activation, squash;
};

__device__ __forceinline__ double policy_activation(double y, int activation) {
  return activation == PIC_ACT_TANH ? tanh(y) : (y > 0.0 ? y : 0.0);
}

// y_i = b_i, then y_i = y_i + W[i][k] h[k] for k ascending: the product rounded, then the sum (the translation unit is built with
// -ffp-contract=off).  Every lane walks its own row of W; the rows of one layer are read by every workgroup and stay in L2.
// (The compiler requests 8 weights at a time.  Requesting 32 was measured and is not built: no faster at 256 environments,
// 5 us slower at 1024, where its 102 registers halve the workgroups in flight: profiles/policy_rollout.md.)
__device__ __forceinline__ double policy_row(const double* __restrict__ W, const double* __restrict__ b,
                                             const double* __restrict__ hin, int i, int nin) {
  const double* __restrict__ w = W + (size_t)i * nin;
  double y = b[i];
  for (int k = 0; k < nin; ++k) y = y + w[k] * hin[k];
  return y;
}

// One workgroup per environment.  The observation is mesh_mode's with modes_kernel's workgroup shape (the bits of pic_get_modes),
// the two activation vectors live in LDS, the weights stream from global memory.
__global__ __launch_bounds__(BLOCK) void policy_kernel(PolicyArgs a) {
  __shared__ double ws[2 * WAVES];
  __shared__ double hbuf[2][kPolicyMaxWidth];
  const int env = blockIdx.x, t = threadIdx.x;
  const int n0 = 2 * a.Mo;
  if (a.obs) {
    if (t < n0) hbuf[0][t] = a.obs[(size_t)env * n0 + t];
  } else {
    const double* __restrict__ E = a.E_mesh + (size_t)env * a.Ng;
    for (int m = 0; m < a.Mo; ++m) {
      double re, im;
      mesh_mode<WAVES>(E, a.tw + (size_t)m * a.Ng, a.tw + ((size_t)a.rows + m) * a.Ng, a.Ng, ws, re, im);
      if (t == 0) { hbuf[0][m] = re; hbuf[0][a.Mo + m] = im; }
    }
  }
  __syncthreads();
  if (t < n0) {                       // (each lane rewrites its own element: no barrier between the read and the write)
    const double o = hbuf[0][t];
    if (a.obs_out) a.obs_out[(size_t)env * n0 + t] = o;
    if (a.obs_scale) hbuf[0][t] = o * a.obs_scale[t];
  }
  __syncthreads();
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const int width[kPolicyMaxLayers + 1] = {a.w0, a.w1, a.w2, a.w3, a.w4};
  int cur = 0;
#pragma unroll
  for (int l = 0; l < kPolicyMaxLayers; ++l) {
    if (l >= a.n_layers) break;       // (uniform: every lane of the workgroup takes the same layers and barriers)
    const int nin = width[l], nout = width[l + 1];
    const double* __restrict__ W = p;
    const double* __restrict__ b = p + (size_t)nout * nin;
    p = b + nout;
    if (l + 1 < a.n_layers) {
      if (t < nout) hbuf[cur ^ 1][t] = policy_activation(policy_row(W, b, hbuf[cur], t, nin), a.activation);
      __syncthreads();
      cur ^= 1;
      continue;
    }
    if (t < nout) {
      const double z = policy_row(W, b, hbuf[cur], t, nin);
      const size_t at = (size_t)env * nout + t;
      double u = z;
      if (a.noise) {
        const double sd = a.std ? a.std[t] : 1.0;
        const double e = sd * a.noise[at];
        u = z + e;
      }
      const double act = a.squash ? a.action_scale * tanh(u) : u;
      if (a.pre_out) a.pre_out[at] = u;
      if (a.act) a.act[at] = act;
      if (a.act_out) a.act_out[at] = act;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The policy's vector-Jacobian product (pic_policy_vjp, pic_tape_backward_policy; include/picstep.h)
// ---------------------------------------------------------------------------------------------
// One evaluation of the VJP for every environment.  Pointers are those of environment 0 (and of the step the launch is for).
struct PolicyVjpArgs {
  const double* obs;         // [env][2 Mo] the recorded observation (before obs_scale)
  const double* obs_scale;   // [2 Mo] or null
  const double* params;      // as PolicyArgs
  const double* pre;         // [env][nA] the recorded u, or null (squash == 0)
  const double* cot_a;       // [env][nA] a cotangent on the action, or null: 0 (gext null)
  const double* gext;        // [env][Ng] e-bar of the step, or null: the cotangent on the action is then B^T e-bar, not cot_a
  const double* basis;       // [2][Ng][M] the actuator's tables (gext)
  const double* cot_a2;      // [env][nA] a second one, added to the first (the caller's direct cotangent), or null
  const double* cot_obs;     // [env][2 Mo] a direct cotangent on the observation: m-bar = o-bar + cot_obs, or null
  double* g_params;          // [env][P] per-environment sums: g = g + term (first: g = term)
  double* g_obs;             // [env][2 Mo] o-bar, or null
  double* g_pre;             // [env][nA] u-bar, or null
  double* g_act;             // [env][nA] the reported a-bar (+ cot_a2), or null
  double* mbar;              // [env][2 Mo] the o-bar that goes on into the plasma, + cot_obs; or null
  long long env_params;      // doubles from one environment's parameters to the next (0: shared)
  long long P;               // doubles of one parameter vector
  double action_scale;
  int first;                 // this launch starts the sums of g_params
  int Ng;                    // (gext)
  int Mo, n_layers;
  int w0, w1, w2, w3, w4;
  int activation, squash;
};

// One backward sweep through the layers from the delta in ds[0] (a barrier behind its write), ending in a barrier.  REP: the sweep
// of the reported a-bar: it adds the parameter terms and writes g_obs.  PROP: the sweep whose o-bar goes on: it writes mbar.
template <bool REP, bool PROP>
__device__ __forceinline__ void policy_vjp_sweep(const PolicyVjpArgs& a, const double* __restrict__ p0,
                                                 const double (*hs)[kPolicyMaxWidth], double (*ds)[kPolicyMaxWidth], int env, int t) {
  const int width[kPolicyMaxLayers + 1] = {a.w0, a.w1, a.w2, a.w3, a.w4};
  const int L = a.n_layers, n0 = a.w0;
  long long off[kPolicyMaxLayers];    // where each layer's W starts in the parameter vector
  {
    long long at = 0;
#pragma unroll
    for (int l = 0; l < kPolicyMaxLayers; ++l) {
      off[l] = at;
      at += (long long)width[l + 1] * width[l] + width[l + 1];
    }
  }
  double* __restrict__ g = a.g_params + (size_t)env * a.P;
  int cur = 0;
#pragma unroll
  for (int l = kPolicyMaxLayers - 1; l >= 0; --l) {
    if (l >= L) continue;               // (uniform)
    const int nin = width[l], nout = width[l + 1];
    const double* __restrict__ W = p0 + off[l];
    const double* __restrict__ delta = ds[cur];
    const double* __restrict__ hin = hs[l];
    if (REP) {
      double* __restrict__ gW = g + off[l];
      double* __restrict__ gb = gW + (size_t)nout * nin;
      if (t < nout) gb[t] = a.first ? delta[t] : gb[t] + delta[t];
      for (int at = t; at < nout * nin; at += BLOCK) {      // (at most 65536: an int)
        const int i = at / nin, k = at - i * nin;
        const double term = delta[i] * hin[k];
        gW[at] = a.first ? term : gW[at] + term;
      }
    }
    if (t < nin) {
      double s = W[t] * delta[0];
      for (int i = 1; i < nout; ++i) s = s + W[(size_t)i * nin + t] * delta[i];
      if (l > 0) {
        const double hv = hin[t];
        const double dact = a.activation == PIC_ACT_TANH ? 1.0 - hv * hv : (hv > 0.0 ? 1.0 : 0.0);
        ds[cur ^ 1][t] = s * dact;
      } else {
        const double ob = a.obs_scale ? s * a.obs_scale[t] : s;
        const size_t at = (size_t)env * n0 + t;
        if (REP && a.g_obs) a.g_obs[at] = ob;
        if (PROP && a.mbar) a.mbar[at] = a.cot_obs ? ob + a.cot_obs[at] : ob;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
}

// One workgroup per environment.  The forward is recomputed with policy_row / policy_activation (the forward's bits): thread i
// owns row i.  Backwards thread k owns column k of W^T delta, so consecutive lanes read consecutive W[i][k]; the parameter terms
// delta_i h_k are one read-modify-write of the environment's own [P] block, element idx by thread idx % BLOCK: no two lanes, and
// no two workgroups, touch one sum.  The activations of every layer and two delta vectors live in LDS.
__global__ __launch_bounds__(BLOCK) void policy_vjp_kernel(PolicyVjpArgs a) {
  __shared__ double hs[kPolicyMaxLayers][kPolicyMaxWidth];      // h_0 .. h_{L-1}
  __shared__ double ds[2][kPolicyMaxWidth];
  const int env = blockIdx.x, t = threadIdx.x;
  const int width[kPolicyMaxLayers + 1] = {a.w0, a.w1, a.w2, a.w3, a.w4};
  const int n0 = a.w0, L = a.n_layers;
  if (t < n0) {
    const double o = a.obs[(size_t)env * n0 + t];
    hs[0][t] = a.obs_scale ? o * a.obs_scale[t] : o;
  }
  __syncthreads();
  const double* __restrict__ p0 = a.params + (size_t)env * a.env_params;
  {
    const double* __restrict__ p = p0;
#pragma unroll
    for (int l = 0; l < kPolicyMaxLayers - 1; ++l) {
      if (l + 1 >= L) break;            // (uniform)
      const int nin = width[l], nout = width[l + 1];
      const double* __restrict__ W = p;
      const double* __restrict__ b = p + (size_t)nout * nin;
      p = b + nout;
      if (t < nout) hs[l + 1][t] = policy_activation(policy_row(W, b, hs[l], t, nin), a.activation);
      __syncthreads();
    }
  }
  const int nA = L == 1 ? a.w1 : (L == 2 ? a.w2 : (L == 3 ? a.w3 : a.w4));
  // Inside a reverse pass (gext) a-bar = B^T e-bar is formed twice, as the gain law's backward forms it:
  // ab_rep with adjoint_actions_kernel's sum (the mesh ascending, from 0.0) is the a-bar that is reported and that the parameter
  // gradient, u-bar and o-bar follow from; ab_prop with law_adjoint_kernel's sum (lanes strided by 64, then wave_sum) is the
  // one whose o-bar goes on into the plasma, so that a linear policy continues the law's reverse pass bit for bit.  The two
  // differ in rounding only.  One wave per coefficient makes both from the same rounded products: each lane adds its own to
  // the strided sum, and every lane adds all 64 of a chunk in lane order (readlane with a uniform index) to the ascending one.
  // Outside a reverse pass (pic_policy_vjp) there is one a-bar and one sweep.
  double ab_rep = 0.0, ab_prop = 0.0, sq = 1.0;
  if (a.gext) {
    const double* __restrict__ g = a.gext + (size_t)env * a.Ng;
    const int lane = t & 63, Mh = nA / 2;
    for (int m = t >> 6; m < nA; m += WAVES) {          // (uniform within a wave)
      const double* __restrict__ b = a.basis + (m < Mh ? 0 : (size_t)a.Ng * Mh);
      const int mm = m < Mh ? m : m - Mh;
      double strided = 0.0, ascending = 0.0;
      for (int base = 0; base < a.Ng; base += 64) {
        const int j = base + lane;
        double p = 0.0;
        if (j < a.Ng) {
          p = b[(size_t)j * Mh + mm] * g[j];
          strided += p;
        }
        const int cnt = a.Ng - base < 64 ? a.Ng - base : 64;
        for (int l = 0; l < cnt; ++l)
          ascending += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(p), l),
                                        __builtin_amdgcn_readlane(__double2loint(p), l));
      }
      strided = wave_sum(strided);
      if (lane == 0) { ds[0][m] = ascending; ds[1][m] = strided; }      // (both free until the first sweep's delta goes there)
    }
    __syncthreads();
    if (t < nA) { ab_rep = ds[0][t]; ab_prop = ds[1][t]; }
    __syncthreads();
  } else if (t < nA && a.cot_a) {
    ab_rep = ab_prop = a.cot_a[(size_t)env * nA + t];
  }
  if (t < nA) {
    const size_t at = (size_t)env * nA + t;
    if (a.cot_a2) {
      ab_rep = ab_rep + a.cot_a2[at];
      ab_prop = ab_prop + a.cot_a2[at];
    }
    if (a.squash) {
      const double th = tanh(a.pre[at]);
      sq = a.action_scale * (1.0 - th * th);
    }
    if (a.g_act) a.g_act[at] = ab_rep;
    if (a.g_pre) a.g_pre[at] = a.squash ? ab_rep * sq : ab_rep;
    ds[0][t] = a.squash ? ab_rep * sq : ab_rep;
  }
  __syncthreads();
  if (!a.gext) {                        // (uniform)
    policy_vjp_sweep<true, true>(a, p0, hs, ds, env, t);
    return;
  }
  policy_vjp_sweep<true, false>(a, p0, hs, ds, env, t);
  if (t < nA) ds[0][t] = a.squash ? ab_prop * sq : ab_prop;
  __syncthreads();
  policy_vjp_sweep<false, true>(a, p0, hs, ds, env, t);
}

// g [P] = the per-environment sums gE [env][P] added in ascending environment order, the first starting the sum: one thread per
// parameter
__global__ __launch_bounds__(256) void policy_grad_reduce_kernel(const double* __restrict__ gE, double* __restrict__ g,
                                                                 long long P, int num_envs) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  double s = gE[p];
  for (int e = 1; e < num_envs; ++e) s = s + gE[(size_t)e * P + p];
  g[p] = s;
}

// ---------------------------------------------------------------------------------------------
// The policy's Jacobian-vector product (pic_policy_jvp, pic_tape_tangent_policy; include/picstep.h)
// ---------------------------------------------------------------------------------------------
// One evaluation of the JVP for every (environment, direction).  Pointers are those of environment 0 and direction 0 (and of the
// step the launch is for); every per-direction array carries its own distance, in doubles, from one direction's row to the next.
struct PolicyJvpArgs {
  const double* obs;         // [env][2 Mo] the recorded observation (before obs_scale)
  const double* obs_scale;   // [2 Mo] or null
  const double* params;      // as PolicyArgs
  const double* pre;         // [env][nA] the recorded u, or null (squash == 0)
  const double* d_params;    // [K][P] or [K][env][P] the parameters' tangent, or null: 0
  const double* d_obs;       // [K][env][2 Mo] the observation's tangent (before obs_scale), or null: 0
  const double* d_pre;       // [K][env][nA] added to du (the caller's d_std * eps), or null
  const double* d_act;       // [K][env][nA] added to da behind the squash (a step's d_actions), or null
  double* du;                // [K][env][nA] du, or null
  double* da;                // [K][env][nA] da, or null
  long long dparams_stride, dobs_stride, dpre_stride, dact_stride, du_stride, da_stride;
  long long env_params;      // doubles from one environment's parameters (and their tangent) to the next (0: shared)
  double action_scale;
  int n_layers;
  int w0, w1, w2, w3, w4;
  int activation, squash;
};

// One workgroup per (environment, direction): blockIdx.y is the direction.  Carrying the directions of an environment in one
// workgroup would recompute the forward once instead of K times, but the forward is the smaller half of a layer's work here, and
// at 256 environments K workgroups per environment are what fills the device.  Thread i owns row i of a layer,
// for the forward (policy_row: the forward's bits) and for the tangent; h_l, h_{l+1} and their tangents live in LDS.
//   dy_i = db_i;  k ascending: dy_i = dy_i + dW[i][k] * h[k];  k ascending: dy_i = dy_i + W[i][k] * dh[k].
__global__ __launch_bounds__(BLOCK) void policy_jvp_kernel(PolicyJvpArgs a) {
  __shared__ double hbuf[2][kPolicyMaxWidth];
  __shared__ double dbuf[2][kPolicyMaxWidth];
  const int env = blockIdx.x, d = blockIdx.y, t = threadIdx.x;
  const int width[kPolicyMaxLayers + 1] = {a.w0, a.w1, a.w2, a.w3, a.w4};
  const int n0 = a.w0, L = a.n_layers;
  if (t < n0) {
    const double o = a.obs[(size_t)env * n0 + t];
    const double dob = a.d_obs ? a.d_obs[(size_t)d * a.dobs_stride + (size_t)env * n0 + t] : 0.0;
    hbuf[0][t] = a.obs_scale ? o * a.obs_scale[t] : o;
    dbuf[0][t] = a.obs_scale ? dob * a.obs_scale[t] : dob;
  }
  __syncthreads();
  const double* __restrict__ p = a.params + (size_t)env * a.env_params;
  const double* __restrict__ dp = a.d_params ? a.d_params + (size_t)d * a.dparams_stride + (size_t)env * a.env_params : nullptr;
  int cur = 0;
#pragma unroll
  for (int l = 0; l < kPolicyMaxLayers; ++l) {
    if (l >= L) break;                  // (uniform)
    const int nin = width[l], nout = width[l + 1];
    const size_t nW = (size_t)nout * nin;
    const bool last = l + 1 == L;
    if (t < nout) {
      const double* __restrict__ hin = hbuf[cur];
      const double* __restrict__ dh = dbuf[cur];
      const double* __restrict__ w = p + (size_t)t * nin;
      double dy = 0.0;
      if (dp) {
        const double* __restrict__ dw = dp + (size_t)t * nin;
        dy = dp[nW + t];
        for (int k = 0; k < nin; ++k) dy = dy + dw[k] * hin[k];
      }
      for (int k = 0; k < nin; ++k) dy = dy + w[k] * dh[k];
      if (!last) {
        const double hv = policy_activation(policy_row(p, p + nW, hin, t, nin), a.activation);
        const double dact = a.activation == PIC_ACT_TANH ? 1.0 - hv * hv : (hv > 0.0 ? 1.0 : 0.0);
        hbuf[cur ^ 1][t] = hv;
        dbuf[cur ^ 1][t] = dy * dact;
      } else {
        const size_t at = (size_t)env * nout + t;
        double du = dy;
        if (a.d_pre) du = dy + a.d_pre[(size_t)d * a.dpre_stride + at];
        double da = du;
        if (a.squash) {
          const double th = tanh(a.pre[at]);
          da = (a.action_scale * (1.0 - th * th)) * du;
        }
        if (a.d_act) da = da + a.d_act[(size_t)d * a.dact_stride + at];
        if (a.du) a.du[(size_t)d * a.du_stride + at] = du;
        if (a.da) a.da[(size_t)d * a.da_stride + at] = da;
      }
    }
    if (last) break;
    __syncthreads();
    p += nW + nout;
    if (dp) dp += nW + nout;
    cur ^= 1;
  }
}

}  // namespace
