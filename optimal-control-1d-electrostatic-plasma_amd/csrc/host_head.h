// host_head.h -- what a call of either controller has in common, the MLP policy's (host_policy.h) and the particle actor's
// (host_actor.h): a flat parameter vector, optional noise / std, the outputs pre and actions, one own row per step
// (the observation, the feature row) and optionally nsteps closed-loop steps with the energies' record.
// Included by picstep.hip inside its extern "C" block, in front of host_policy.h and behind the stepping entries (advance); its
// first part has no HIP and no pic_handle, and tests/head_driver.cpp pins it on a CPU (tests/test_head_cpu.py).
#pragma once

#include <cstddef>

#include "picstep.h"

extern "C++" {
constexpr int kHeadMaxWidth = 256, kHeadPolicyLayers = 4, kHeadActorLayers = 6;      // (pic_policy.h, pic_actor.h; asserted below)

// P, the doubles of one parameter vector: per layer W [out][in] and b [out] and -- with layernorm, behind every layer but the
// last -- gamma [out] and beta [out]
static size_t head_param_count(const int* width, int n_layers, bool layernorm) {
  size_t P = 0;
  for (int l = 0; l < n_layers; ++l) {
    const size_t nout = (size_t)width[l + 1];
    P += nout * (size_t)width[l] + nout + (layernorm && l + 1 < n_layers ? 2 * nout : 0);
  }
  return P;
}

// What is wrong with mem_kind and the fields that pic_policy and pic_actor both have (s: one of them), or null.  own(slot) is the
// caller's own check (a message or null) at the four places where the two controllers have one, so that a call with several
// faults reports the one it always did.
enum { kOwnBehindMemKind, kOwnBehindLayers, kOwnBehindWidths, kOwnBehindFlags };
template <typename Spec, typename Own>
static const char* head_bad_shape(const Spec& s, int mem_kind, int max_layers, Own own) {
  if (mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) return "bad mem_kind";
  if (const char* bad = own(kOwnBehindMemKind)) return bad;
  if (s.n_layers < 1 || s.n_layers > max_layers) return max_layers == kHeadPolicyLayers ? "n_layers must be 1..4" : "n_layers must be 1..6";
  if (const char* bad = own(kOwnBehindLayers)) return bad;
  for (int l = 0; l <= s.n_layers; ++l)
    if (s.width[l] < 1 || s.width[l] > kHeadMaxWidth) return "every width must be 1..256";
  if (const char* bad = own(kOwnBehindWidths)) return bad;
  if (s.activation != PIC_ACT_TANH && s.activation != PIC_ACT_RELU) return "activation must be PIC_ACT_TANH or PIC_ACT_RELU";
  if (s.squash != 0 && s.squash != 1) return "squash must be 0 or 1";
  if (s.per_env != 0 && s.per_env != 1) return "per_env must be 0 or 1";
  if (const char* bad = own(kOwnBehindFlags)) return bad;
  return s.params ? nullptr : "null params";
}

#ifdef __HIPCC__      // ---- from here on: the handle and the stream ----------------------------------------------------------------
static_assert(kPolicyMaxWidth == kHeadMaxWidth && kPolicyMaxLayers == kHeadPolicyLayers && kActorMaxLayers == kHeadActorLayers,
              "head_bad_shape's messages name these limits");

// the actuator a controller acts through: PIC_ESTATE without one, PIC_EINVAL if the last width is not its 2M
static int head_actuator(pic_handle* h, int last_width, const char* who) {
  if (!h->act_modes) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_set_actuator first");
  if (last_width != 2 * h->act_modes)
    return fail(h, PIC_EINVAL, std::string(who) + ": the last width must be 2 max_mode of the actuator (pic_set_actuator) = " +
                                   std::to_string(2 * h->act_modes));
  return PIC_OK;
}

// How an entry that does not step opens (p: a pic_policy or a pic_actor; bad: what its argument check says, from a handle that is
// not null).  Its own refusals and hipSetDevice follow.
template <typename Spec>
static int head_entry(pic_handle* h, const Spec* p, const char* bad, const char* who) {
  if (!h) return PIC_EINVAL;
  if (bad) return fail(h, PIC_EINVAL, std::string(who) + ": " + bad);
  return head_actuator(h, p->width[p->n_layers], who);
}

// One call's arguments, whichever the controller (row_out: the rows of its own output, obs_out or features_out)
struct HeadCall {
  const double *noise, *std;
  int mem_kind, nsteps;
  bool stepping;
  double *row_out, *pre_out, *actions_out, *hist;
};

// the own row of a controller's argument block: the member that points at it, and its doubles per environment
template <typename Args>
struct HeadRow {
  double* Args::*out;
  size_t width;
};

// The common inputs of a call on the device and the common members of the argument block of its first step (k: a HeadCall on
// the views of its block; d: P, per_env and the handle's dims)
template <typename Call, typename Args>
static int head_stage(pic_handle* h, const Call& k, const double* params, const BlockDims& d, Args& a) {
  const size_t D = sizeof(double);
  HIPCHK(h, device_input(h, params, k.mem_kind, d.params() * D, k.d_params, &a.params));
  HIPCHK(h, device_input(h, k.std, k.mem_kind, 2 * d.act_modes * D, k.d_std, &a.std));
  HIPCHK(h, device_input(h, k.noise, k.mem_kind, (size_t)k.nsteps * d.arow() * D, k.d_noise, &a.noise));
  a.pre_out = device_output(k.pre_out, k.mem_kind, k.d_pre_out);
  if (k.stepping) {
    a.act = k.d_act;
    a.act_out = k.mem_kind == PIC_DEVICE ? k.actions_out : nullptr;      // (host: the rows themselves are read back)
  } else {
    a.act = device_output(k.actions_out, k.mem_kind, k.d_act);
  }
  a.env_params = d.per_env ? (long long)d.P : 0;
  return PIC_OK;
}

// The closed loop.  Step s: launch(the argument block of step s) evaluates the controller on what step s-1 left, its own row
// into row s of its rows and its actions into row s of the actions; then the step pic_step_actions(row s, 1) makes.  No row is
// written twice within a call, so the launches of step s+1 cannot overtake a force evaluation of step s.
template <typename Args, typename Launch>
static int head_steps(pic_handle* h, StepControl& sc, const Args& a0, HeadRow<Args> row, int nsteps, double* d_hist, Launch launch) {
  const size_t E = (size_t)h->cfg.num_envs, ra = E * 2 * (size_t)h->act_modes;
  Args a = a0;
  int rc = PIC_OK;
  for (int s = 0; s < nsteps && rc == PIC_OK; ++s) {
    launch(a);
    sc.ctl.act = a.act;
    rc = advance(h, sc, 1, hist_at(h, d_hist, (size_t)s));
    if (a.noise) a.noise += ra;      // the argument block of the next step: every per-step row moved on by one step
    if (a.*row.out) a.*row.out += E * row.width;
    if (a.pre_out) a.pre_out += ra;
    if (a.act) a.act += ra;
    if (a.act_out) a.act_out += ra;
  }
  return rc;
}

// the read-backs of a call in host memory and of the energies' record; one wait, if anything is read back (after a failed step
// too: what was enqueued is waited for)
template <typename Call, typename Args>
static int head_finish(pic_handle* h, const Call& k, const Args& a0, HeadRow<Args> row, const char* who) {
  const size_t E = (size_t)h->cfg.num_envs, rows = (size_t)k.nsteps * E * sizeof(double), nA = 2 * (size_t)h->act_modes;
  hipError_t e = hipGetLastError();
  bool wait = false;
  if (k.mem_kind == PIC_HOST) {
    if (e == hipSuccess) e = device_result(h, k.row_out, a0.*row.out, rows * row.width);
    if (e == hipSuccess) e = device_result(h, k.pre_out, a0.pre_out, rows * nA);
    if (e == hipSuccess) e = device_result(h, k.actions_out, a0.act, rows * nA);
    wait = k.row_out || k.pre_out || k.actions_out;
  }
  if (k.hist) {
    if (e == hipSuccess) e = hipMemcpyAsync(k.hist, k.d_hist, rows * 3, hipMemcpyDeviceToHost, h->stream);
    wait = true;
  }
  return hip_tail(h, e, wait, who);
}
#endif
}  // extern "C++"
