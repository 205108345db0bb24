// host_blocks.h -- the layouts of every carved device block: no HIP, no pic_handle.  Included by host_diff.h (picstep.hip) and by
// tests/blocks_driver.cpp, which pins every byte total and offset on a CPU (tests/test_blocks_cpu.py).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "pic_limits.h"

namespace {      // internal linkage throughout: the library exports its C ABI alone

// A device block cut into parts, every part rounded up to 256 bytes.  A block is described once, by a layout function below that
// take()s its parts in order into the views of a holder and returns `at`, the block's bytes: with base = null it only sizes the
// block, with the block's address it assigns the views.  A part without elements gets no view (null).
struct Carver {
  char* base = nullptr;
  size_t at = 0;
  static size_t rounded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  template <typename T>
  void take(T*& view, size_t count) {
    take_tail(view, count);
    at = rounded(at);
  }
  // a part that ends its block where its elements end, unrounded (the two blocks that have one say why)
  template <typename T>
  void take_tail(T*& view, size_t count) {
    if (base) view = count ? reinterpret_cast<T*>(base + at) : nullptr;
    at += count * sizeof(T);
  }
  // bytes of consecutive parts: from the start of the first to `end`, the end of the last one's elements, rounded
  static size_t upto(const void* first, const void* end) {
    return rounded((size_t)(static_cast<const char*>(end) - static_cast<const char*>(first)));
  }
};

// What the layouts read of a handle (host_diff.h: block_dims), of a policy (host_policy.h: policy_dims) and of the phase JVP
struct BlockDims {
  size_t num_envs = 0, ld = 0, Ng = 0, act_modes = 0;
  size_t P = 0, obs_modes = 0;        // the policy's: doubles of one parameter vector, observed modes
  bool per_env = false;               // ... a parameter vector per environment
  size_t chunks = 0;                  // the phase JVP's chunks per environment (host_phase.h: phase_jvp_chunks)
  size_t part() const { return num_envs * ld; }
  size_t mesh() const { return num_envs * Ng; }
  size_t arow() const { return num_envs * 2 * act_modes; }
  size_t orow() const { return num_envs * 2 * obs_modes; }
  size_t params() const { return (per_env ? num_envs : 1) * P; }
};

// ---- the tape (host_tape.h) -----------------------------------------------------------------------------------
struct TapeViews {
  double* ck = nullptr;               // [nck][2][env][ld] checkpoints: (x, v) before step c * every
  double* ext = nullptr;              // [max_steps][env][Ng] e_t
  double* seg = nullptr;              // [every + 1][2][env][ld] one segment's replayed states
  double* F = nullptr;                // [every][3][env][Ng] its sub-stage fields
  double* M = nullptr;                // [every][env][Ng] its post-step fields
  double* lam = nullptr;              // [2][env][ld] lambda_q, lambda_p
  double* cot = nullptr;              // [max_steps][3][env] energy cotangents
  double* gext = nullptr;             // [max_steps][env][Ng] e-bar
  double* nu = nullptr;               // [env][Ng]
  long long* acc = nullptr;           // [env][Ng] (acc_t) zero between uses
  unsigned long long* cmax = nullptr; // [env] zero between uses, and the two counters behind it
  double* gact = nullptr;             // [max_steps][env][2M] a-bar (M: the actuator's modes at pic_tape_start; none without one)
};

// the parts of the block of a tape of max_steps steps with a checkpoint every `every` steps
inline size_t tape_parts(Carver c, const BlockDims& d, int64_t max_steps, int64_t every, TapeViews& t) {
  const size_t E = d.num_envs, part = d.part(), mesh = d.mesh(), T = (size_t)max_steps, ev = (size_t)every;
  c.take(t.ck, (size_t)(max_steps / every + 1) * 2 * part);
  c.take(t.ext, T * mesh);
  c.take(t.seg, (ev + 1) * 2 * part);
  c.take(t.F, ev * 3 * mesh);
  c.take(t.M, ev * mesh);
  c.take(t.lam, 2 * part);
  c.take(t.cot, T * 3 * E);
  c.take(t.gext, T * mesh);
  c.take(t.nu, mesh);
  c.take(t.acc, mesh);
  c.take(t.cmax, E + 2);
  c.take(t.gact, T * d.arow());
  return c.at;
}

// the record of the gain law's steps (pic_step_feedback_gain)
struct LawViews {
  double* act = nullptr;              // [max_steps][env][2M] a_t of the law's steps (their e_t = B a_t goes to `ext` behind the call)
  double* modes = nullptr;            // [max_steps][env][2M] m_t of the law's steps, zero on the others
  double* cot = nullptr;              // [max_steps][env][2M] cotangents on m_t of a backward
  double* E = nullptr;                // [env][Ng] E-bar_t = J^T (G^T a-bar_t + m-bar_t) of a law step
};

inline size_t law_parts(Carver c, const BlockDims& d, int64_t max_steps, LawViews& v) {
  const size_t rows = (size_t)max_steps * d.arow();
  c.take(v.act, rows);
  c.take(v.modes, rows);
  c.take(v.cot, rows);
  c.take_tail(v.E, d.mesh());         // unrounded: pic_tape_info.bytes has always counted this block so, and the totals are pinned
  return c.at;
}

// the per-step smoothed KL (pic_tape_kl_start) for nx x nv bins
struct KlViews {
  double* feq = nullptr;              // [nx][nv] or [env][nx][nv] the tape's copy of the target
  unsigned long long* acc = nullptr;  // [env][nx][nv] integer sums, zero between uses
  double* g = nullptr;                // [env][nx][nv] cotangent grid of the step being reversed
  double* trace = nullptr;            // [max_steps][env] KL~ after every step
  double* cot = nullptr;              // [max_steps][env] cotangents on it (pic_tape_kl_cot)
};

inline size_t tape_kl_parts(Carver c, const BlockDims& d, int nx, int nv, bool feq_per_env, int64_t max_steps, KlViews& v) {
  const size_t E = d.num_envs, nb2 = (size_t)nx * nv, rows = (size_t)max_steps * E;
  c.take(v.feq, (feq_per_env ? E : 1) * nb2);
  c.take(v.acc, E * nb2);
  c.take(v.g, E * nb2);
  c.take(v.trace, rows);
  c.take(v.cot, rows);
  return c.at;
}

// cotangents on the moments of the tape's states (pic_tape_moments_cot): [max_steps + 1][env][3][Ng], row s + 1 for
// the state step s left, row 0 for the tape start
struct MomCotViews { double* cot = nullptr; };

inline size_t tape_moments_parts(Carver c, const BlockDims& d, int64_t max_steps, MomCotViews& v) {
  c.take(v.cot, (size_t)(max_steps + 1) * 3 * d.mesh());
  return c.at;
}

// the moments of every taped step (pic_tape_moments_start): [max_steps][env][3][Ng], row t of the state step t left
struct MomTraceViews { double* trace = nullptr; };

inline size_t tape_moments_trace_parts(Carver c, const BlockDims& d, int64_t max_steps, MomTraceViews& v) {
  c.take(v.trace, (size_t)max_steps * 3 * d.mesh());
  return c.at;
}

// steps under an MLP policy (pic_tape_step_policy); d: the policy's dims
struct TapePolicyViews {
  double* obs = nullptr;              // [max_steps][env][2 Mo] o_t of the policy's steps
  double* pre = nullptr;              // [max_steps][env][2M] u_t
  double* act = nullptr;              // [max_steps][env][2M] a_t (their e_t = B a_t goes to `ext` as an actions step's)
  double* gobs = nullptr;             // [max_steps][env][2 Mo] o-bar_t of the last reverse pass, zero on the other steps
  double* gpre = nullptr;             // [max_steps][env][2M] u-bar_t
  double* gact = nullptr;             // [max_steps][env][2M] a-bar_t = B^T e-bar_t + the direct cotangent
  double* cobs = nullptr;             // [max_steps][env][2 Mo] direct cotangents on o_t of a backward
  double* cact = nullptr;             // [max_steps][env][2M] direct cotangents on a_t of a backward
  double* mbar = nullptr;             // [env][2 Mo] m-bar of the step being reversed
  double* gE = nullptr;               // [env][P] the parameter gradient's per-environment sums
  double* g = nullptr;                // [P] their sum in ascending environment order (shared parameters)
};

inline size_t tape_policy_parts(Carver c, const BlockDims& d, int64_t max_steps, TapePolicyViews& v) {
  const size_t T = (size_t)max_steps, orows = T * d.orow(), arows = T * d.arow();
  c.take(v.obs, orows);
  c.take(v.pre, arows);
  c.take(v.act, arows);
  c.take(v.gobs, orows);              // (gobs, gpre, gact: cleared as one range by walk_open)
  c.take(v.gpre, arows);
  c.take(v.gact, arows);
  c.take(v.cobs, orows);
  c.take(v.cact, arows);
  c.take(v.mbar, d.orow());
  c.take(v.gE, d.num_envs * d.P);
  c.take(v.g, d.per_env ? 0 : d.P);
  return c.at;
}

// a policy call's copy on the tape: params [P] or [env][P], obs_scale [2 Mo] behind them
struct PolicyCopyViews { double *params = nullptr, *scale = nullptr; };

inline size_t policy_copy_parts(Carver c, const BlockDims& d, bool has_scale, PolicyCopyViews& v) {
  c.take(v.params, d.params());
  c.take_tail(v.scale, 2 * d.obs_modes);    // unrounded, and there without an obs_scale too: the pinned totals count the copy so
  if (!has_scale) v.scale = nullptr;
  return c.at;
}

// ---- forward mode of the tape (host_tangent.h) --------------------------------------------------------------
// the tangent block for kc directions into a holder with TanArgs' members (pic_tangent.h): state [kc][2][env][ld], dF
// [kc][env][Ng], acc [kc][env][Ng], ke [kc][env], umax [3][kc][env] (everything from acc on is zero between uses)
template <typename Holder>
size_t tangent_parts(Carver c, const BlockDims& d, int kc, Holder& ta) {
  const size_t E = d.num_envs, k = (size_t)kc;
  c.take(ta.st, k * 2 * d.part());
  c.take(ta.dF, k * d.mesh());
  c.take(ta.acc, k * d.mesh());
  c.take(ta.ke, k * E);
  c.take(ta.umax, 3 * k * E);
  return c.at;
}

// the block behind the KL's tangent for kc directions: the unit cotangents [env] (the finishing kernel's g is then dKL~/df) and
// the chunks' sums [kc][env][chunks] of the step at hand
struct TanKlViews { double *ones = nullptr, *part = nullptr; };

inline size_t tangent_kl_parts(Carver c, const BlockDims& d, int kc, TanKlViews& v) {
  c.take(v.ones, d.num_envs);
  c.take(v.part, (size_t)kc * d.num_envs * d.chunks);
  return c.at;
}

// ---- the moments (host_moments.h) --------------------------------------------------------------------------------
// the handle's block: the integer sums [3][env][Ng], the max words [env] (both zero between calls) and the device copy [env][3][Ng]
// of a result that goes to host memory
struct MomViews {
  unsigned long long *acc = nullptr, *max = nullptr;
  double* out = nullptr;
};

inline size_t moments_parts(Carver c, const BlockDims& d, MomViews& v) {
  c.take(v.acc, 3 * d.mesh());
  c.take(v.max, d.num_envs);
  c.take(v.out, 3 * d.mesh());
  return c.at;
}

// the forward mode's working memory for kc directions into a holder with MomJvpArgs' members (pic_moments.h): the integer sums
// [3][kc][env][Ng] and the max words [3][kc][env] (zero between uses)
template <typename Holder>
size_t moments_jvp_parts(Carver c, const BlockDims& d, int kc, Holder& j) {
  c.take(j.acc, (size_t)3 * kc * d.mesh());
  c.take(j.umax, (size_t)3 * kc * d.num_envs);
  return c.at;
}

// ---- pooled particle features (host_pool.h) ----------------------------------------------------------------
// what a pic_pool / pic_pool_vjp / pic_pool_jvp call (or its _ln form) gives and wants, as far as its block depends on it
struct PoolCallShape {
  size_t H = 0, N = 0;                // hidden units; particles per environment
  bool per_env = false;               // a parameter vector per environment
  bool vjp = false;                   // pic_pool_vjp (else pic_pool)
  bool host = false, params_host = false;               // the call's arrays, its parameters: in host memory
  bool xv = false;                    // x and v are given (else the handle's particles)
  bool g_x = false, g_v = false, g_params = false;      // outputs wanted (vjp)
  bool ln = false;                    // pic_pool_ln / pic_pool_ln_vjp: P = 6H (W, b, gamma, beta), two max words in the VJP
  bool jvp = false;                   // pic_pool_jvp / pic_pool_ln_jvp (vjp is false then)
  int K = 0;                          // ... its directions
  bool d_x = false, d_v = false, d_params = false;      // ... the tangents given
};

// the handle's block: the max words [env] (the LayerNorm's VJP and JVP: r_max [env] behind them; the JVP: the tangents' maxima
// [2][K][env] behind those) and the integer sums [env][H], [env][P] or [K][env][H] (all zero between calls), the VJP's
// per-environment parameter sums and -- for what lives in host memory -- the device copies of the call's inputs and outputs
struct PoolViews {
  unsigned long long *max = nullptr, *acc = nullptr;
  double *gE = nullptr, *params = nullptr, *x = nullptr, *v = nullptr, *cot = nullptr, *out = nullptr, *g_x = nullptr,
         *g_v = nullptr, *g = nullptr;
  unsigned long long* tmax = nullptr;                   // the JVP's [2][K][env] inside `max`
  double *d_params = nullptr, *d_x = nullptr, *d_v = nullptr;      // the JVP's tangents given in host memory (out: d_out)
};

inline size_t pool_parts(Carver c, const BlockDims& d, const PoolCallShape& s, PoolViews& k) {
  const size_t E = d.num_envs, P = (s.ln ? 6 : 4) * s.H, rows = E * s.N, K = s.jvp ? (size_t)s.K : 1;
  const size_t own = s.ln && (s.vjp || s.jvp) ? 2 * E : E;      // (u_max, and r_max where a bound needs it)
  c.take(k.max, own + (s.jvp ? 2 * K * E : 0));
  if (s.jvp && k.max) k.tmax = k.max + own;
  c.take(k.acc, E * (s.vjp ? P : K * s.H));
  // (shared parameters: the rows the reduction reads; per-environment ones in device memory are written where the caller wants them)
  c.take(k.gE, s.vjp && s.g_params && (!s.per_env || s.host) ? E * P : 0);
  c.take(k.params, s.params_host ? (s.per_env ? E : 1) * P : 0);
  c.take(k.d_params, s.jvp && s.d_params && s.params_host ? K * (s.per_env ? E : 1) * P : 0);
  if (!s.host) return c.at;
  c.take(k.x, s.xv ? rows : 0);
  c.take(k.v, s.xv ? rows : 0);
  c.take(k.cot, s.vjp ? E * s.H : 0);
  c.take(k.out, s.vjp ? 0 : K * E * s.H);
  c.take(k.g_x, s.g_x ? rows : 0);
  c.take(k.g_v, s.g_v ? rows : 0);
  c.take(k.g, s.g_params && !s.per_env ? P : 0);
  c.take(k.d_x, s.jvp && s.d_x ? K * rows : 0);
  c.take(k.d_v, s.jvp && s.d_v ? K * rows : 0);
  return c.at;
}

// The passes' launch: a workgroup walks chunks_per_wg consecutive chunks of kPoolChunkTiles tiles (2 particles each), and
// `workgroups` of them cover an environment.  About 4096 workgroups of 4 waves in all: the passes are bound by tanh and sincos,
// and a workgroup holds 8 KB of LDS at most.
constexpr long long kPoolChunkTiles = 512;      // (pic_pool.h: POOL_BLOCK * kPoolTiles; host_pool.h asserts it)
struct PoolPlan { long long chunks_per_wg = 0, workgroups = 0; };

inline PoolPlan pool_plan(size_t num_envs, size_t N) {
  const long long E = (long long)num_envs, ntiles = ((long long)N + 1) / 2, nchunks = (ntiles + kPoolChunkTiles - 1) / kPoolChunkTiles;
  const long long wpe = std::max(1LL, std::min((4096 + E - 1) / E, nchunks));
  PoolPlan p;
  p.chunks_per_wg = (nchunks + wpe - 1) / wpe;
  p.workgroups = (nchunks + p.chunks_per_wg - 1) / p.chunks_per_wg;
  return p;
}

// The recorder's particle pass (pic_record.h: record_hist_kernel), planned at pic_record_start; tests/record_plan_driver.cpp and
// tests/test_record_edges_cpu.py pin it.  Geometry: about 1024 workgroups in all, gx per environment, each over a contiguous
// range of tiles_per_wg tile columns (a column: one 16-byte tile of `vec` particles per lane).  LDS: rr copies of each marginal
// bin within 32 KiB, then the word of `inside`, then the phase histogram in rows of pv + 1 words where all of it fits
// kRecordLdsBytes (phase_lds); global atomics otherwise.  Counts are integers: no result depends on any of it.
constexpr int kRecordLdsBytes = 64 << 10;       // LDS of the particle pass: sub-histograms up to this size live in LDS
struct RecordPlan {
  int gx = 1;
  long long tiles_per_wg = 1;
  int rr = 1, phase_lds = 0;
  size_t lds = 0;
};

inline RecordPlan record_plan(long long N, long long vec, int E, int xb, int vb, int px, int pv) {
  RecordPlan p;
  const long long cols = ((N + vec - 1) / vec + BLOCK - 1) / BLOCK;     // tiles per lane if one workgroup took it all
  const long long gx = std::max(1LL, std::min(cols, (1024LL + E - 1) / E));
  p.tiles_per_wg = (cols + gx - 1) / gx;
  p.gx = (int)((cols + p.tiles_per_wg - 1) / p.tiles_per_wg);
  int rr = 16;
  while (rr > 1 && (size_t)rr * (xb + vb) * sizeof(unsigned) > ((size_t)32 << 10)) rr /= 2;
  p.rr = rr;
  const size_t marg = ((size_t)rr * (xb + vb) + 1) * sizeof(unsigned), prow = (size_t)px * (pv + 1) * sizeof(unsigned);
  p.phase_lds = marg + prow <= (size_t)kRecordLdsBytes ? 1 : 0;
  p.lds = marg + (p.phase_lds ? prow : 0);
  return p;
}

// ---- forward mode through closed loops (host_tangent_walk.h) ------------------------------------------------------
// the working rows of a walk of kc directions observing mo modes: the field tangent the last step left dM [kc][env][Ng], its
// energies' tangents [kc][3][env], the observation's tangent [kc][env][2 mo], the law's dm [kc][env][2M], the action tangent of
// the step at hand da [kc][env][2M], dG [kc][env][2M][2M], and a step's injection from host memory
struct TanWalkViews { double *dM = nullptr, *hist = nullptr, *obs = nullptr, *dm = nullptr, *da = nullptr, *dG = nullptr, *in = nullptr; };

inline size_t tanwalk_parts(Carver c, const BlockDims& d, int kc, int mo, TanWalkViews& v) {
  const size_t E = d.num_envs, mesh = d.mesh(), arow = d.arow(), k = (size_t)kc;
  c.take(v.dM, k * mesh);
  c.take(v.hist, k * 3 * E);
  c.take(v.obs, k * E * 2 * mo);
  c.take(v.dm, k * arow);
  c.take(v.da, k * arow);
  c.take(v.dG, k * arow * 2 * d.act_modes);
  c.take(v.in, k * std::max(mesh, arow));
  return c.at;
}

// the working rows of a walk through the policy's steps for kc directions (d: the policy's dims): the parameters' tangent dtheta
// [kc][P] or [kc][env][P], the du of the step at hand [kc][env][2M], and a step's d_pre from host memory
struct TanPolViews { double *dtheta = nullptr, *du = nullptr, *pin = nullptr; };

inline size_t tanpol_parts(Carver c, const BlockDims& d, int kc, TanPolViews& v) {
  const size_t k = (size_t)kc;
  c.take(v.dtheta, k * d.params());
  c.take(v.du, k * d.arow());
  c.take(v.pin, k * d.arow());
  return c.at;
}

// ---- the handle's policy block (host_policy.h), one call's parts at a time; d: the policy's dims ----------
// what a call gives and wants, as far as its block depends on it
struct PolicyCallShape {
  size_t nsteps = 1;
  bool host = false, stepping = false;
  bool scale = false, std = false, noise = false, obs = false, pre = false;   // inputs given
  bool obs_out = false, pre_out = false, actions_out = false, hist = false;   // outputs wanted
  bool d_params = false, d_obs = false, d_pre = false;                        // tangents given (pic_policy_jvp)
};

// pic_policy_eval, pic_step_policy, pic_tape_step_policy: the per-step rows of the actions the steps read, the energies' record,
// and -- for a call in host memory -- the device copies of its inputs and outputs
struct PolicyCallViews {
  double *d_act = nullptr, *d_hist = nullptr, *d_params = nullptr, *d_scale = nullptr, *d_std = nullptr, *d_noise = nullptr,
         *d_obs = nullptr, *d_obs_out = nullptr, *d_pre_out = nullptr;
};

inline size_t policy_parts(Carver c, const BlockDims& d, const PolicyCallShape& s, PolicyCallViews& k) {
  const size_t T = s.nsteps, orow = d.orow(), arow = d.arow();
  c.take(k.d_act, s.stepping ? T * arow : (s.host && s.actions_out ? arow : 0));
  c.take(k.d_hist, s.hist ? T * 3 * d.num_envs : 0);
  if (!s.host) return c.at;
  c.take(k.d_params, d.params());
  c.take(k.d_scale, s.scale ? 2 * d.obs_modes : 0);
  c.take(k.d_std, s.std ? 2 * d.act_modes : 0);
  c.take(k.d_noise, s.noise ? T * arow : 0);
  c.take(k.d_obs, s.obs ? orow : 0);
  c.take(k.d_obs_out, s.obs_out ? T * orow : 0);
  c.take(k.d_pre_out, s.pre_out ? T * arow : 0);
  return c.at;
}

// ---- the particle actor's calls on the same block (host_actor.h); d: the head's dims (P, per_env) ------------------
struct ActorCallShape {
  size_t nsteps = 1, H = 0;           // steps of the call (pic_actor_eval: 1); the pool's hidden units
  bool host = false, stepping = false;
  bool particles = false;             // the feature rows come from the pool's sums (else: features are given)
  bool std = false, noise = false;                                            // inputs given
  bool features_out = false, pre_out = false, actions_out = false, hist = false;      // outputs wanted
};

// pic_actor_eval, pic_step_actor: the per-step rows of the actions the steps read, the feature rows the kernel writes where they
// do not go straight to the caller's device memory (a row feeds the head, so there always is one where the sums are finished),
// the energies' record, and -- for a call in host memory -- the device copies of its inputs and outputs
struct ActorCallViews {
  double *d_act = nullptr, *d_feat = nullptr, *d_hist = nullptr, *d_params = nullptr, *d_std = nullptr, *d_noise = nullptr,
         *d_features = nullptr, *d_pre_out = nullptr;
};

inline size_t actor_parts(Carver c, const BlockDims& d, const ActorCallShape& s, ActorCallViews& k) {
  const size_t T = s.nsteps, frow = d.num_envs * s.H, arow = d.arow();
  const bool to_caller = !s.host && s.features_out;       // the kernel writes the caller's rows itself
  c.take(k.d_act, s.stepping ? T * arow : (s.host && s.actions_out ? arow : 0));
  c.take(k.d_feat, (s.particles ? !to_caller : s.host && s.features_out) ? T * frow : 0);
  c.take(k.d_hist, s.hist ? T * 3 * d.num_envs : 0);
  if (!s.host) return c.at;
  c.take(k.d_params, d.params());
  c.take(k.d_std, s.std ? 2 * d.act_modes : 0);
  c.take(k.d_noise, s.noise ? T * arow : 0);
  c.take(k.d_features, s.particles ? 0 : frow);
  c.take(k.d_pre_out, s.pre_out ? T * arow : 0);
  return c.at;
}

// pic_policy_vjp: the per-environment sums, their reduction, and -- in host memory -- the copies of its inputs and outputs
struct PolicyVjpViews {
  double *gE = nullptr, *g = nullptr, *params = nullptr, *scale = nullptr, *obs = nullptr, *pre = nullptr, *cot = nullptr,
         *g_obs = nullptr, *g_pre = nullptr;
};

inline size_t policy_vjp_parts(Carver c, const BlockDims& d, const PolicyCallShape& s, PolicyVjpViews& k) {
  const size_t orow = d.orow(), arow = d.arow();
  c.take(k.gE, d.num_envs * d.P);
  c.take(k.g, d.per_env ? 0 : d.P);
  if (!s.host) return c.at;
  c.take(k.params, d.params());
  c.take(k.scale, s.scale ? 2 * d.obs_modes : 0);
  c.take(k.obs, orow);
  c.take(k.pre, s.pre ? arow : 0);
  c.take(k.cot, arow);
  c.take(k.g_obs, s.obs_out ? orow : 0);
  c.take(k.g_pre, s.pre_out ? arow : 0);
  return c.at;
}

// pic_policy_jvp in host memory, K directions: the copies of its inputs and outputs (pre_out: du, actions_out: da)
struct PolicyJvpViews {
  double *params = nullptr, *scale = nullptr, *obs = nullptr, *pre = nullptr, *d_params = nullptr, *d_obs = nullptr, *d_pre = nullptr,
         *du = nullptr, *da = nullptr;
};

inline size_t policy_jvp_parts(Carver c, const BlockDims& d, const PolicyCallShape& s, int K, PolicyJvpViews& k) {
  const size_t orow = d.orow(), arow = d.arow(), kk = (size_t)K;
  c.take(k.params, d.params());
  c.take(k.scale, s.scale ? 2 * d.obs_modes : 0);
  c.take(k.obs, orow);
  c.take(k.pre, s.pre ? arow : 0);
  c.take(k.d_params, s.d_params ? kk * d.params() : 0);
  c.take(k.d_obs, s.d_obs ? kk * orow : 0);
  c.take(k.d_pre, s.d_pre ? kk * arow : 0);
  c.take(k.du, s.pre_out ? kk * arow : 0);
  c.take(k.da, s.actions_out ? kk * arow : 0);
  return c.at;
}

}  // namespace
