// host_policy.h -- the host side of pic_policy_eval and pic_step_policy (kernel: pic_policy.h).
// Included by picstep.hip inside its extern "C" block, behind the stepping entries (step_prologue, actuator_control, advance).

// P, the doubles of one parameter vector
static size_t policy_param_count(const pic_policy* p) {
  size_t P = 0;
  for (int l = 0; l < p->n_layers; ++l) P += (size_t)p->width[l + 1] * p->width[l] + p->width[l + 1];
  return P;
}

// what is wrong with a policy whatever the actuator, or null
static const char* policy_bad_args(const pic_handle* h, const pic_policy* p, int mem_kind) {
  if (!p) return "null policy";
  if (mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) return "bad mem_kind";
  if (p->n_layers < 1 || p->n_layers > kPolicyMaxLayers) return "n_layers must be 1..4";
  if (p->obs_modes < 1 || p->obs_modes > kPolicyMaxObsModes) return "obs_modes must be 1..64";
  if (p->obs_modes >= h->cfg.Ng) return "obs_modes must be below N_mesh";
  for (int l = 0; l <= p->n_layers; ++l)
    if (p->width[l] < 1 || p->width[l] > kPolicyMaxWidth) return "every width must be 1..256";
  if (p->width[0] != 2 * p->obs_modes) return "width[0] must be 2 obs_modes";
  if (p->activation != PIC_ACT_TANH && p->activation != PIC_ACT_RELU) return "activation must be PIC_ACT_TANH or PIC_ACT_RELU";
  if (p->squash != 0 && p->squash != 1) return "squash must be 0 or 1";
  if (p->per_env != 0 && p->per_env != 1) return "per_env must be 0 or 1";
  if (!p->params) return "null params";
  return nullptr;
}

// the actuator a policy acts through: PIC_ESTATE without one, PIC_EINVAL if the last width is not its 2M
static int policy_actuator(pic_handle* h, const pic_policy* p, const char* who) {
  if (!h->act_modes) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_set_actuator first");
  if (p->width[p->n_layers] != 2 * h->act_modes)
    return fail(h, PIC_EINVAL, std::string(who) + ": the last width must be 2 max_mode of the actuator (pic_set_actuator) = " +
                                   std::to_string(2 * h->act_modes));
  return PIC_OK;
}

// One call's arguments, and the views into the handle's policy block it works on (h->pol): the per-step rows of the actions the
// steps read, the energies' record, and -- for a call in host memory -- the device copies of its inputs and outputs.
struct PolicyCall {
  const pic_policy* p;
  const double *obs, *noise, *std;
  int mem_kind, nsteps;
  bool stepping;
  double *obs_out, *pre_out, *actions_out, *hist;
  // views
  double *d_act = nullptr, *d_hist = nullptr, *d_params = nullptr, *d_scale = nullptr, *d_std = nullptr, *d_noise = nullptr,
         *d_obs = nullptr, *d_obs_out = nullptr, *d_pre_out = nullptr;
};

static size_t policy_parts(Carver& c, PolicyCall& k, const pic_handle* h) {
  const size_t E = (size_t)h->cfg.num_envs, T = (size_t)k.nsteps;
  const size_t nO = 2 * (size_t)k.p->obs_modes, nA = 2 * (size_t)h->act_modes;
  const bool host = k.mem_kind == PIC_HOST;
  c.take(k.d_act, k.stepping ? T * E * nA : (host && k.actions_out ? E * nA : 0));
  c.take(k.d_hist, k.hist ? T * 3 * E : 0);
  if (!host) return c.at;
  c.take(k.d_params, (k.p->per_env ? E : 1) * policy_param_count(k.p));
  c.take(k.d_scale, k.p->obs_scale ? nO : 0);
  c.take(k.d_std, k.std ? nA : 0);
  c.take(k.d_noise, k.noise ? T * E * nA : 0);
  c.take(k.d_obs, k.obs ? E * nO : 0);
  c.take(k.d_obs_out, k.obs_out ? T * E * nO : 0);
  c.take(k.d_pre_out, k.pre_out ? T * E * nA : 0);
  return c.at;
}

// The block of a call, its inputs on the device and the argument block of its first step (the per-step pointers at row 0)
static int policy_begin(pic_handle* h, PolicyCall& k, PolicyArgs& a) {
  Carver size;
  PolicyCall scratch = k;
  const size_t bytes = policy_parts(size, scratch, h);
  if (bytes > h->pol_bytes) {
    h->pol_bytes = 0;
    const int rc = regrow(h, h->pol, bytes, "the policy's device block does not fit on the device");
    if (rc) return rc;
    h->pol_bytes = bytes;
  }
  Carver c;
  c.base = static_cast<char*>(h->pol.get());
  policy_parts(c, k, h);
  const pic_policy* p = k.p;
  const size_t E = (size_t)h->cfg.num_envs, T = (size_t)k.nsteps, D = sizeof(double);
  const size_t nO = 2 * (size_t)p->obs_modes, nA = 2 * (size_t)h->act_modes, P = policy_param_count(p);
  a = PolicyArgs{};
  HIPCHK(h, device_input(h, p->params, k.mem_kind, (p->per_env ? E : 1) * P * D, k.d_params, &a.params));
  HIPCHK(h, device_input(h, p->obs_scale, k.mem_kind, nO * D, k.d_scale, &a.obs_scale));
  HIPCHK(h, device_input(h, k.std, k.mem_kind, nA * D, k.d_std, &a.std));
  HIPCHK(h, device_input(h, k.noise, k.mem_kind, T * E * nA * D, k.d_noise, &a.noise));
  HIPCHK(h, device_input(h, k.obs, k.mem_kind, E * nO * D, k.d_obs, &a.obs));
  if (!k.obs) {
    const int rc = ensure_twiddle(h, p->obs_modes);
    if (rc) return rc;
  }
  a.E_mesh = h->E_mesh; a.tw = h->tw; a.rows = h->tw_rows; a.Ng = h->cfg.Ng;
  a.obs_out = device_output(k.obs_out, k.mem_kind, k.d_obs_out);
  a.pre_out = device_output(k.pre_out, k.mem_kind, k.d_pre_out);
  if (k.stepping) {
    a.act = k.d_act;
    a.act_out = k.mem_kind == PIC_DEVICE ? k.actions_out : nullptr;      // (host: the rows themselves are read back)
  } else {
    a.act = device_output(k.actions_out, k.mem_kind, k.d_act);
  }
  a.env_params = p->per_env ? (long long)P : 0;
  a.action_scale = p->action_scale;
  a.Mo = p->obs_modes; a.n_layers = p->n_layers;
  a.w0 = p->width[0]; a.w1 = p->width[1]; a.w2 = p->width[2]; a.w3 = p->width[3]; a.w4 = p->width[4];
  a.activation = p->activation; a.squash = p->squash;
  return PIC_OK;
}

// the argument block of step s: every per-step row moved on by s steps
static PolicyArgs policy_at(const PolicyArgs& a0, size_t s, size_t E, size_t nA) {
  PolicyArgs a = a0;
  const size_t ro = s * E * 2 * (size_t)a.Mo, ra = s * E * nA;
  if (a.noise) a.noise += ra;
  if (a.obs_out) a.obs_out += ro;
  if (a.pre_out) a.pre_out += ra;
  if (a.act) a.act += ra;
  if (a.act_out) a.act_out += ra;
  return a;
}

static void policy_launch(pic_handle* h, const PolicyArgs& a) {
  hipLaunchKernelGGL(policy_kernel, dim3(h->cfg.num_envs), dim3(BLOCK), 0, h->stream, a);
}

// the read-backs of a call in host memory and of the energies' record; one wait, if anything is read back
static int policy_finish(pic_handle* h, const PolicyCall& k, const PolicyArgs& a0, const char* who) {
  const size_t E = (size_t)h->cfg.num_envs, T = (size_t)k.nsteps, D = sizeof(double);
  const size_t nO = 2 * (size_t)k.p->obs_modes, nA = 2 * (size_t)h->act_modes;
  hipError_t e = hipGetLastError();
  bool wait = false;
  if (k.mem_kind == PIC_HOST) {
    if (e == hipSuccess) e = device_result(h, k.obs_out, a0.obs_out, T * E * nO * D);
    if (e == hipSuccess) e = device_result(h, k.pre_out, a0.pre_out, T * E * nA * D);
    if (e == hipSuccess) e = device_result(h, k.actions_out, a0.act, T * E * nA * D);
    wait = k.obs_out || k.pre_out || k.actions_out;
  }
  if (k.hist) {
    if (e == hipSuccess) e = hipMemcpyAsync(k.hist, k.d_hist, T * 3 * E * D, hipMemcpyDeviceToHost, h->stream);
    wait = true;
  }
  const hipError_t e2 = wait ? hipStreamSynchronize(h->stream) : hipSuccess;
  if (e != hipSuccess || e2 != hipSuccess)
    return fail(h, PIC_EHIP, std::string(who) + ": " + hipGetErrorString(e != hipSuccess ? e : e2));
  return PIC_OK;
}

int pic_policy_eval(pic_handle* h, const pic_policy* p, const double* obs, const double* noise, const double* std, int mem_kind,
                    double* obs_out, double* pre_out, double* actions_out) {
  const char* who = "pic_policy_eval";
  if (!h) return PIC_EINVAL;
  if (const char* bad = policy_bad_args(h, p, mem_kind)) return fail(h, PIC_EINVAL, std::string(who) + ": " + bad);
  int rc = policy_actuator(h, p, who);
  if (rc) return rc;
  if (!obs && !h->has_state) return fail(h, PIC_ESTATE, std::string(who) + ": call pic_reset first (obs = NULL reads the current E_mesh)");
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  PolicyCall k{p, obs, noise, std, mem_kind, 1, false, obs_out, pre_out, actions_out, nullptr};
  PolicyArgs a;
  rc = policy_begin(h, k, a);
  if (rc) return rc;
  policy_launch(h, a);
  return policy_finish(h, k, a, who);
}

int pic_step_policy(pic_handle* h, const pic_policy* p, const double* noise, const double* std, int mem_kind, int nsteps,
                    double* obs_out, double* pre_out, double* actions_out, double* hist) {
  const char* who = "pic_step_policy";
  if (h && h->tape.on)
    return fail(h, PIC_ESTATE, "pic_step_policy: refused while a tape is open (its actions depend on the state: the gradient through the policy would be missing)");
  int rc = step_prologue(h, nsteps, who, h ? policy_bad_args(h, p, mem_kind) : nullptr);
  if (rc) return rc;
  rc = policy_actuator(h, p, who);
  if (rc || nsteps == 0) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, who);
  if (rc) return rc;
  PolicyCall k{p, nullptr, noise, std, mem_kind, nsteps, true, obs_out, pre_out, actions_out, hist};
  PolicyArgs a0;
  rc = policy_begin(h, k, a0);
  if (rc) return rc;
  // Step s: the policy on the field step s-1 left, into row s of the actions; then the step pic_step_actions(row s, 1) makes.
  // No row is written twice within a call, so the policy launch of step s+1 cannot overtake a force evaluation of step s.
  const int E = h->cfg.num_envs;
  for (int s = 0; s < nsteps && rc == PIC_OK; ++s) {
    const PolicyArgs a = policy_at(a0, (size_t)s, (size_t)E, 2 * (size_t)h->act_modes);
    policy_launch(h, a);
    sc.ctl.act = a.act;
    rc = advance(h, sc, 1, hist_at(h, k.d_hist, (size_t)s));
  }
  const int rf = policy_finish(h, k, a0, who);      // (after a failed step too: what was enqueued is waited for)
  return rc ? rc : rf;
}
