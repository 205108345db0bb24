// host_policy.h -- the host side of pic_policy_eval, pic_step_policy, pic_policy_vjp and pic_tape_step_policy (7p) and pic_policy_jvp (7q); kernels: pic_policy.h.
// Included by picstep.hip inside its extern "C" block, behind the stepping entries (step_prologue, actuator_control) and
// host_head.h, which holds what a call shares with the particle actor's (host_actor.h); the layouts of its blocks are
// host_blocks.h's, call_reserve and tape_reserve (host_diff.h) allocate them.

// the policy's dims (host_blocks.h: BlockDims)
static BlockDims policy_dims(const pic_handle* h, const pic_policy& p) {
  BlockDims d = block_dims(h);
  d.P = head_param_count(p.width, p.n_layers, false); d.obs_modes = (size_t)p.obs_modes; d.per_env = p.per_env != 0;
  return d;
}

// what is wrong with a policy whatever the actuator, or null: head_bad_shape and, at their places, the checks of its observation
static const char* policy_bad_args(const pic_handle* h, const pic_policy* p, int mem_kind) {
  if (!p) return "null policy";
  return head_bad_shape(*p, mem_kind, kPolicyMaxLayers, [&](int slot) -> const char* {
    if (slot == kOwnBehindLayers) {
      if (p->obs_modes < 1 || p->obs_modes > kPolicyMaxObsModes) return "obs_modes must be 1..64";
      if (p->obs_modes >= h->cfg.Ng) return "obs_modes must be below N_mesh";
    }
    if (slot == kOwnBehindWidths && p->width[0] != 2 * p->obs_modes) return "width[0] must be 2 obs_modes";
    return nullptr;
  });
}

// One call's arguments on the views into the handle's policy block it works on (host_blocks.h: policy_parts)
struct PolicyCall : PolicyCallViews, HeadCall {
  const pic_policy* p;
  const double* obs;
};
static HeadRow<PolicyArgs> policy_row(const pic_policy* p) { return {&PolicyArgs::obs_out, 2 * (size_t)p->obs_modes}; }

// The block of a call, its inputs on the device and the argument block of its first step (the per-step pointers at row 0)
static int policy_begin(pic_handle* h, PolicyCall& k, PolicyArgs& a, const char* who) {
  const pic_policy* p = k.p;
  const BlockDims d = policy_dims(h, *p);
  PolicyCallShape s;
  s.nsteps = (size_t)k.nsteps; s.host = k.mem_kind == PIC_HOST; s.stepping = k.stepping;
  s.scale = p->obs_scale; s.std = k.std; s.noise = k.noise; s.obs = k.obs;
  s.obs_out = k.row_out; s.pre_out = k.pre_out; s.actions_out = k.actions_out; s.hist = k.hist;
  if (int rc = call_reserve<PolicyCallViews>(h, h->pol, &h->pol_bytes, who, "the policy's device block", k,
                                             [&](Carver c, PolicyCallViews& v) { return policy_parts(c, d, s, v); }))
    return rc;
  a = PolicyArgs{};
  if (int rc = head_stage(h, k, p->params, d, a)) return rc;
  HIPCHK(h, device_input(h, p->obs_scale, k.mem_kind, 2 * d.obs_modes * sizeof(double), k.d_scale, &a.obs_scale));
  HIPCHK(h, device_input(h, k.obs, k.mem_kind, d.orow() * sizeof(double), k.d_obs, &a.obs));
  if (!k.obs) {
    const int rc = ensure_twiddle(h, p->obs_modes);
    if (rc) return rc;
  }
  a.E_mesh = h->E_mesh; a.tw = h->tw; a.rows = h->tw_rows; a.Ng = h->cfg.Ng;
  a.obs_out = device_output(k.row_out, k.mem_kind, k.d_obs_out);
  a.Mo = p->obs_modes;
  policy_shape(a, *p, d.P, p->action_scale);
  return PIC_OK;
}

static void policy_launch(pic_handle* h, const PolicyArgs& a) {
  hipLaunchKernelGGL(policy_kernel, dim3(h->cfg.num_envs), dim3(BLOCK), 0, h->stream, a);
}

int pic_policy_eval(pic_handle* h, const pic_policy* p, const double* obs, const double* noise, const double* std, int mem_kind,
                    double* obs_out, double* pre_out, double* actions_out) {
  const char* who = "pic_policy_eval";
  int rc = head_entry(h, p, h ? policy_bad_args(h, p, mem_kind) : nullptr, who);
  if (rc) return rc;
  if (!obs && !h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first (obs = NULL reads the current E_mesh)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  PolicyCall k{{}, {noise, std, mem_kind, 1, false, obs_out, pre_out, actions_out, nullptr}, p, obs};
  PolicyArgs a;
  rc = policy_begin(h, k, a, who);
  if (rc) return rc;
  policy_launch(h, a);
  return head_finish(h, k, a, policy_row(p), who);
}

// ---- the policy's vector-Jacobian product (pic_policy_vjp; kernel: pic_policy.h) ---------------------------------
int pic_policy_vjp(pic_handle* h, const pic_policy* p, const double* obs, const double* pre, const double* cot_actions, int mem_kind,
                   double* g_params, double* g_obs, double* g_pre) {
  const char* who = "pic_policy_vjp";
  int rc = head_entry(h, p, h ? policy_bad_args(h, p, mem_kind) : nullptr, who);
  if (rc) return rc;
  if (!obs || !cot_actions) return fail(h, PIC_EINVAL, std::string(who) + ": null obs or cot_actions");
  if (!pre && p->squash) return fail(h, PIC_EINVAL, std::string(who) + ": pre may be NULL only with squash == 0");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const bool host = mem_kind == PIC_HOST;
  const BlockDims d = policy_dims(h, *p);
  PolicyCallShape s;
  s.host = host; s.scale = p->obs_scale; s.pre = pre; s.obs_out = g_obs; s.pre_out = g_pre;
  PolicyVjpViews k;
  rc = call_reserve(h, h->pol, &h->pol_bytes, who, "the policy's device block", k,
                    [&](Carver c, PolicyVjpViews& v) { return policy_vjp_parts(c, d, s, v); });
  if (rc) return rc;
  const size_t E = d.num_envs, D = sizeof(double), P = d.P, nO = 2 * d.obs_modes, nA = 2 * d.act_modes;
  PolicyVjpArgs a{};
  HIPCHK(h, device_input(h, p->params, mem_kind, (p->per_env ? E : 1) * P * D, k.params, &a.params));
  HIPCHK(h, device_input(h, p->obs_scale, mem_kind, nO * D, k.scale, &a.obs_scale));
  HIPCHK(h, device_input(h, obs, mem_kind, E * nO * D, k.obs, &a.obs));
  HIPCHK(h, device_input(h, pre, mem_kind, E * nA * D, k.pre, &a.pre));
  HIPCHK(h, device_input(h, cot_actions, mem_kind, E * nA * D, k.cot, &a.cot_a));
  a.g_params = k.gE;
  a.g_obs = device_output(g_obs, mem_kind, k.g_obs);
  a.g_pre = device_output(g_pre, mem_kind, k.g_pre);
  a.P = (long long)P;
  a.first = 1;
  a.Mo = p->obs_modes;
  policy_shape(a, *p, P, p->action_scale);
  hipLaunchKernelGGL(policy_vjp_kernel, dim3(h->cfg.num_envs), dim3(BLOCK), 0, h->stream, a);
  const double* gsrc = k.gE;
  if (!p->per_env && g_params) {
    hipLaunchKernelGGL(policy_grad_reduce_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, (const double*)k.gE, k.g,
                       (long long)P, h->cfg.num_envs);
    gsrc = k.g;
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && g_params)
    e = hipMemcpyAsync(g_params, gsrc, (p->per_env ? E : 1) * P * D, copy_kind(mem_kind, hipMemcpyDeviceToHost), h->stream);
  if (host) {
    if (e == hipSuccess) e = device_result(h, g_obs, a.g_obs, E * nO * D);
    if (e == hipSuccess) e = device_result(h, g_pre, a.g_pre, E * nA * D);
  }
  return hip_tail(h, e, host, who);
}

// ---- the policy's Jacobian-vector product (pic_policy_jvp; kernel: pic_policy.h) ---------------------------------
int pic_policy_jvp(pic_handle* h, const pic_policy* p, const double* obs, const double* pre, int K, const double* d_params,
                   const double* d_obs, const double* d_pre, int mem_kind, double* d_pre_out, double* d_actions_out) {
  const char* who = "pic_policy_jvp";
  int rc = head_entry(h, p, h ? policy_bad_args(h, p, mem_kind) : nullptr, who);
  if (rc) return rc;
  if (K < 1 || K > kMaxTangents) return fail(h, PIC_EINVAL, std::string(who) + ": need 1 <= K <= " + std::to_string(kMaxTangents));
  if (!obs) return fail(h, PIC_EINVAL, std::string(who) + ": null obs");
  if (!pre && p->squash) return fail(h, PIC_EINVAL, std::string(who) + ": pre may be NULL only with squash == 0");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const bool host = mem_kind == PIC_HOST;
  const size_t E = (size_t)h->cfg.num_envs, D = sizeof(double), P = policy_dims(h, *p).P, PE = (p->per_env ? E : 1) * P;
  const size_t nO = 2 * (size_t)p->obs_modes, nA = 2 * (size_t)h->act_modes, kk = (size_t)K;
  PolicyJvpViews k;
  if (host) {
    PolicyCallShape s;
    s.host = true; s.scale = p->obs_scale; s.pre = pre; s.d_params = d_params; s.d_obs = d_obs; s.d_pre = d_pre;
    s.pre_out = d_pre_out; s.actions_out = d_actions_out;
    rc = call_reserve(h, h->pol, &h->pol_bytes, who, "the policy's device block", k,
                      [&](Carver c, PolicyJvpViews& v) { return policy_jvp_parts(c, policy_dims(h, *p), s, K, v); });
    if (rc) return rc;
  }
  PolicyJvpArgs a{};
  HIPCHK(h, device_input(h, p->params, mem_kind, PE * D, k.params, &a.params));
  HIPCHK(h, device_input(h, p->obs_scale, mem_kind, nO * D, k.scale, &a.obs_scale));
  HIPCHK(h, device_input(h, obs, mem_kind, E * nO * D, k.obs, &a.obs));
  HIPCHK(h, device_input(h, pre, mem_kind, E * nA * D, k.pre, &a.pre));
  HIPCHK(h, device_input(h, d_params, mem_kind, kk * PE * D, k.d_params, &a.d_params));
  HIPCHK(h, device_input(h, d_obs, mem_kind, kk * E * nO * D, k.d_obs, &a.d_obs));
  HIPCHK(h, device_input(h, d_pre, mem_kind, kk * E * nA * D, k.d_pre, &a.d_pre));
  a.du = device_output(d_pre_out, mem_kind, k.du);
  a.da = device_output(d_actions_out, mem_kind, k.da);
  a.dparams_stride = (long long)PE;
  a.dobs_stride = (long long)(E * nO);
  a.dpre_stride = a.du_stride = a.da_stride = (long long)(E * nA);
  policy_shape(a, *p, P, p->action_scale);
  hipLaunchKernelGGL(policy_jvp_kernel, dim3(h->cfg.num_envs, K), dim3(BLOCK), 0, h->stream, a);
  hipError_t e = hipGetLastError();
  if (host) {
    if (e == hipSuccess) e = device_result(h, d_pre_out, a.du, kk * E * nA * D);
    if (e == hipSuccess) e = device_result(h, d_actions_out, a.da, kk * E * nA * D);
  }
  return hip_tail(h, e, host, who);
}

// ---- policy steps on an open tape (pic_tape_step_policy) --------------------------------------------------------
static bool policy_same_shape(const pic_policy& a, const pic_policy& b) {
  if (a.obs_modes != b.obs_modes || a.n_layers != b.n_layers || a.activation != b.activation || a.squash != b.squash ||
      a.per_env != b.per_env)
    return false;
  for (int l = 0; l <= a.n_layers; ++l)
    if (a.width[l] != b.width[l]) return false;
  return true;
}

// The policy record of an open tape (allocated by the first policy call) and room for one more call's parameters, within
// budget_bytes; nothing is enqueued or changed when it fails.
static int tape_policy_reserve(pic_handle* h, const pic_policy* p, const char* who) {
  Tape& t = h->tape;
  if (t.policy.block && !policy_same_shape(t.policy.shape, *p))
    return fail(h, PIC_EINVAL, std::string(who) + ": every policy call of one tape must have the same shape (widths, activation, "
                                                  "squash, per_env, obs_modes)");
  const BlockDims d = policy_dims(h, *p);
  const bool first = !t.policy.block;
  PolicyCopyViews cv;
  const size_t cbytes = policy_copy_parts(Carver{}, d, p->obs_scale, cv);
  Tape::Policy::Copy pc;
  const int rc = tape_reserve<TapePolicyViews>(h, t.policy.block, who, "the policy's record and this call's parameters", t.policy,
                                               [&](Carver c, TapePolicyViews& v) { return tape_policy_parts(c, d, t.max_steps, v); },
                                               &pc.params, cbytes, !first);
  if (rc) return rc;
  if (first) {
    t.policy.shape = *p;
    t.policy.shape.params = t.policy.shape.obs_scale = nullptr;
    t.policy.P = d.P;
    t.policy.step.assign((size_t)t.max_steps, -1);
  }
  policy_copy_parts(Carver{reinterpret_cast<char*>(pc.params.get())}, d, p->obs_scale, cv);
  pc.scale = cv.scale;
  pc.action_scale = p->action_scale;
  pc.bytes = cbytes;
  t.policy.calls.push_back(std::move(pc));
  return PIC_OK;
}

int pic_tape_step_policy(pic_handle* h, const pic_policy* p, const double* noise, const double* std, int mem_kind, int nsteps,
                         double* obs_out, double* pre_out, double* actions_out, double* hist) {
  const char* who = "pic_tape_step_policy";
  if (h && !h->tape.on) return fail(h, PIC_ESTATE, "pic_tape_step_policy: no tape is open (pic_tape_start)");
  int rc = step_prologue(h, nsteps, who, h ? policy_bad_args(h, p, mem_kind) : nullptr);
  if (rc) return rc;
  rc = head_actuator(h, p->width[p->n_layers], who);
  if (rc || nsteps == 0) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, who);
  if (rc) return rc;
  Tape& t = h->tape;
  rc = tape_policy_reserve(h, p, who);
  if (rc) return rc;
  // the three records are the tape's rows: the call's own outputs are copied from there behind the steps
  PolicyCall k{{}, {noise, std, mem_kind, nsteps, true, nullptr, nullptr, nullptr, hist}, p, nullptr};
  PolicyArgs a0;
  rc = policy_begin(h, k, a0, who);
  if (rc) {                           // (the copy goes again, and its bytes with it)
    t.bytes -= t.policy.calls.back().bytes;
    t.policy.calls.pop_back();
    return rc;
  }
  const size_t E = (size_t)h->cfg.num_envs, D = sizeof(double), P = t.policy.P;
  const size_t nO = 2 * (size_t)p->obs_modes, nA = 2 * (size_t)h->act_modes, T = (size_t)nsteps;
  const int64_t s0 = t.steps;
  const Tape::Policy::Copy& pc = t.policy.calls.back();
  double* tp = pc.params.get();
  HIPCHK(h, hipMemcpyAsync(tp, a0.params, (p->per_env ? E : 1) * P * D, hipMemcpyDeviceToDevice, h->stream));
  if (pc.scale) HIPCHK(h, hipMemcpyAsync(const_cast<double*>(pc.scale), a0.obs_scale, nO * D, hipMemcpyDeviceToDevice, h->stream));
  a0.params = tp;
  a0.obs_scale = pc.scale;
  a0.obs_out = t.policy.obs + (size_t)s0 * E * nO;
  a0.pre_out = t.policy.pre + (size_t)s0 * E * nA;
  a0.act = t.policy.act + (size_t)s0 * E * nA;
  a0.act_out = nullptr;
  // (as pic_step_policy; advance puts e_t = B a_t on the tape)
  rc = head_steps(h, sc, a0, policy_row(p), nsteps, k.d_hist, [&](const PolicyArgs& a) { policy_launch(h, a); });
  for (int64_t s = s0; s < t.steps; ++s) t.policy.step[(size_t)s] = (int)t.policy.calls.size() - 1;
  const hipMemcpyKind outk = copy_kind(mem_kind, hipMemcpyDeviceToHost);
  hipError_t e = hipSuccess;
  if (e == hipSuccess && obs_out) e = hipMemcpyAsync(obs_out, a0.obs_out, T * E * nO * D, outk, h->stream);
  if (e == hipSuccess && pre_out) e = hipMemcpyAsync(pre_out, a0.pre_out, T * E * nA * D, outk, h->stream);
  if (e == hipSuccess && actions_out) e = hipMemcpyAsync(actions_out, a0.act, T * E * nA * D, outk, h->stream);
  if (e != hipSuccess) return fail(h, PIC_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  const int rf = head_finish(h, k, a0, policy_row(p), who);      // (the energies' record alone: k names no output)
  if (!rf && mem_kind == PIC_HOST && !hist && (obs_out || pre_out || actions_out)) HIPCHK(h, hipStreamSynchronize(h->stream));
  return rc ? rc : rf;
}

int pic_step_policy(pic_handle* h, const pic_policy* p, const double* noise, const double* std, int mem_kind, int nsteps,
                    double* obs_out, double* pre_out, double* actions_out, double* hist) {
  const char* who = "pic_step_policy";
  if (h && h->tape.on)
    return fail(h, PIC_ESTATE, "pic_step_policy: refused while a tape is open (its actions depend on the state: the gradient through the policy would be missing)");
  int rc = step_prologue(h, nsteps, who, h ? policy_bad_args(h, p, mem_kind) : nullptr);
  if (rc) return rc;
  rc = head_actuator(h, p->width[p->n_layers], who);
  if (rc || nsteps == 0) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, who);
  if (rc) return rc;
  PolicyCall k{{}, {noise, std, mem_kind, nsteps, true, obs_out, pre_out, actions_out, hist}, p, nullptr};
  PolicyArgs a0;
  rc = policy_begin(h, k, a0, who);
  if (rc) return rc;
  rc = head_steps(h, sc, a0, policy_row(p), nsteps, k.d_hist, [&](const PolicyArgs& a) { policy_launch(h, a); });
  const int rf = head_finish(h, k, a0, policy_row(p), who);
  return rc ? rc : rf;
}
