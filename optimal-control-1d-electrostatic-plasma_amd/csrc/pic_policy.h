// pic_policy.h -- the MLP policy a = pi(o) on the modes of the mesh field (pic_policy_eval, pic_step_policy).
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

}  // namespace
