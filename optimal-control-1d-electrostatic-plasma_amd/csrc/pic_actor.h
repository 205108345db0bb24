// pic_actor.h -- the DeepSets particle actor a = pi(x, v) (include/picstep.h: pic_actor_eval, pic_step_actor): the
// pooled particle features of pic_pool.h / pic_pool_ln.h, then a head of up to six linear layers with a LayerNorm and an
// activation behind every layer but the last.  One kernel: it finishes the pool's integer sums (pool_finish_body), writes the
// feature row once and runs the head on it.  Included by picstep.hip only.  Built with -ffp-contract=off.
#pragma once

#include "pic_policy.h"
#include "pic_pool_ln.h"

namespace {

constexpr int kActorMaxLayers = 6;
static_assert(POOL_BLOCK >= kPolicyMaxWidth, "one thread per output of a layer");
static_assert(kPoolMaxHidden <= kPolicyMaxWidth, "the feature row is a layer's input");

// where the feature row comes from
constexpr int kActorGiven = 0;           // a.features
constexpr int kActorPool = 1;            // the sums of pool_kernel
constexpr int kActorPoolLn = 2;          // the sums of pool_ln_kernel

// One evaluation of the head for every environment.  Pointers are those of environment 0 (and of the step the launch is for).
struct ActorArgs {
  const double* features;    // [env][H] given features (source == kActorGiven), else null
  const double* params;      // per layer W [out][in] row-major, b [out], and (layernorm, not the last layer) gamma [out], beta [out]
  const double* noise;       // [env][nA] eps, or null
  const double* std;         // [nA], or null: 1
  double* feat_out;          // [env][H] the feature row; never null where the sums are finished (the row feeds the head)
  double* pre_out;           // [env][nA] u, or null
  double* act;               // [env][nA] a, where the step's force evaluations read it, or null
  double* act_out;           // [env][nA] a second copy in the caller's device memory, or null
  long long env_params;      // doubles from one environment's parameters to the next (0: shared)
  double ln_eps, action_scale, action_shift;
  int source, n_layers;
  int w0, w1, w2, w3, w4, w5, w6;      // widths (scalars: an indexed member of the argument block would go through scratch)
  int layernorm, activation, squash;
};

// The LayerNorm of pic_pool_ln over the n values y[0..n) of a layer in LDS, for output t: both sums from +0 over ascending i,
// formed by every thread itself from broadcast reads (no sum is split: the bits do not depend on the launch).
__device__ __forceinline__ double actor_norm(const double* __restrict__ y, int n, int t, double eps, double gamma, double beta) {
  const double nd = (double)n;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = s + y[i];
  const double mu = s / nd;
  double q = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d = y[i] - mu;
    q = q + d * d;
  }
  const double r = 1.0 / sqrt(q / nd + eps);
  const double d = y[t] - mu;
  const double gy = gamma * (d * r);
  return gy + beta;
}

// One workgroup of POOL_BLOCK threads per environment; one thread owns one output of a layer.  The two activation vectors live
// in LDS, the weights stream from global memory (policy_row).  p, n: the pool call's arguments where its sums are finished here.
__global__ __launch_bounds__(POOL_BLOCK) void actor_kernel(ActorArgs a, PoolArgs p, PoolLnArgs n) {
  __shared__ double hbuf[2][kPolicyMaxWidth];
  const int env = blockIdx.x, t = threadIdx.x, n0 = a.w0;
  // the finish of the pool call: the row goes to feat_out, the sums and the max word are cleared (every thread: barriers inside)
  if (a.source == kActorPoolLn) pool_finish_body(p, PoolLn(p, n, env), a.feat_out);
  else if (a.source == kActorPool) pool_finish_body(p, PoolPlain(p, env), a.feat_out);
  if (t < n0) {
    const size_t at = (size_t)env * n0 + t;
    double f;
    if (a.source == kActorGiven) {
      f = a.features[at];
      if (a.feat_out) a.feat_out[at] = f;
    } else {
      f = a.feat_out[at];              // (this thread's own write: H <= POOL_BLOCK, thread k wrote element k)
    }
    hbuf[0][t] = f;
  }
  __syncthreads();
  const double* __restrict__ q = a.params + (size_t)env * a.env_params;
  const int width[kActorMaxLayers + 1] = {a.w0, a.w1, a.w2, a.w3, a.w4, a.w5, a.w6};
  int cur = 0;
#pragma unroll
  for (int l = 0; l < kActorMaxLayers; ++l) {
    if (l >= a.n_layers) break;       // (uniform: every lane of the workgroup takes the same layers and barriers)
    const int nin = width[l], nout = width[l + 1];
    const double* __restrict__ W = q;
    const double* __restrict__ b = q + (size_t)nout * nin;
    q = b + nout;
    if (l + 1 < a.n_layers) {
      if (a.layernorm) {
        // y into the other vector; behind the barrier every thread has read this one, and the normalised row replaces it
        const double* __restrict__ gamma = q;
        const double* __restrict__ beta = q + nout;
        q = beta + nout;
        if (t < nout) hbuf[cur ^ 1][t] = policy_row(W, b, hbuf[cur], t, nin);
        __syncthreads();
        if (t < nout)
          hbuf[cur][t] = policy_activation(actor_norm(hbuf[cur ^ 1], nout, t, a.ln_eps, gamma[t], beta[t]), a.activation);
        __syncthreads();
      } else {
        if (t < nout) hbuf[cur ^ 1][t] = policy_activation(policy_row(W, b, hbuf[cur], t, nin), a.activation);
        __syncthreads();
        cur ^= 1;
      }
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
      double act = u;
      if (a.squash) {
        const double st = a.action_scale * tanh(u);
        act = a.action_shift + st;
      }
      if (a.pre_out) a.pre_out[at] = u;
      if (a.act) a.act[at] = act;
      if (a.act_out) a.act_out[at] = act;
    }
  }
}

}  // namespace
