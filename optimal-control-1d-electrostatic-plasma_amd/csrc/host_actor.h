// host_actor.h -- the host side of pic_actor_eval and pic_step_actor; kernel: pic_actor.h.
// Included by picstep.hip inside its extern "C" block, behind host_policy.h (policy_actuator) and host_pool.h (the pool call that
// a call on particles begins: pool_begin, pool_ln_begin); the layout of its block is host_blocks.h's actor_parts, reserved
// through call_reserve on the handle's policy block.

// P, the doubles of one parameter vector of the head
static size_t actor_param_count(const pic_actor* p) {
  size_t P = 0;
  for (int l = 0; l < p->n_layers; ++l) {
    const size_t nout = (size_t)p->width[l + 1];
    P += nout * (size_t)p->width[l] + nout;
    if (p->layernorm && l + 1 < p->n_layers) P += 2 * nout;
  }
  return P;
}

// what is wrong with an actor whatever the actuator and the source of its features, or null
static const char* actor_bad_args(const pic_actor* p, int mem_kind) {
  if (!p) return "null actor";
  if (mem_kind != PIC_HOST && mem_kind != PIC_DEVICE) return "bad mem_kind";
  if (!p->pool == !p->pool_ln) return "exactly one of pool and pool_ln must be given";
  if (const char* bad = p->pool ? pool_spec_error(p->pool) : pool_ln_spec_error(p->pool_ln)) return bad;
  if (p->n_layers < 1 || p->n_layers > kActorMaxLayers) return "n_layers must be 1..6";
  for (int l = 0; l <= p->n_layers; ++l)
    if (p->width[l] < 1 || p->width[l] > kPolicyMaxWidth) return "every width must be 1..256";
  if (p->width[0] != (p->pool ? p->pool->hidden : p->pool_ln->hidden)) return "width[0] must be the pool's hidden";
  if (p->layernorm != 0 && p->layernorm != 1) return "layernorm must be 0 or 1";
  if (p->activation != PIC_ACT_TANH && p->activation != PIC_ACT_RELU) return "activation must be PIC_ACT_TANH or PIC_ACT_RELU";
  if (p->squash != 0 && p->squash != 1) return "squash must be 0 or 1";
  if (p->per_env != 0 && p->per_env != 1) return "per_env must be 0 or 1";
  if (p->layernorm && !(std::isfinite(p->ln_eps) && p->ln_eps > 0.0)) return "ln_eps must be finite and > 0";
  if (!std::isfinite(p->action_scale) || !std::isfinite(p->action_shift)) return "action_scale and action_shift must be finite";
  if (!p->params) return "null params";
  return nullptr;
}

// policy_actuator for an actor: its rule and its messages on the actor's last width
static int actor_actuator(pic_handle* h, const pic_actor* p, const char* who) {
  pic_policy last{};
  last.n_layers = 1;
  last.width[1] = p->width[p->n_layers];
  return policy_actuator(h, &last, who);
}

// One call's arguments; its base: the views into the handle's policy block it works on (host_blocks.h: actor_parts)
struct ActorCall : ActorCallViews {
  const pic_actor* p;
  const double* features;
  const void *x, *v;
  const double *noise, *std;
  int mem_kind, nsteps;
  bool stepping;
  double *features_out, *pre_out, *actions_out, *hist;
  PoolCall pool;             // the pool call of a call on particles (features == null)
};

// The pool call of a call on particles: pic_pool's / pic_pool_ln's own checks (with their messages), block, zeroing and staging,
// once per call.  Everything is refused before anything is enqueued.
static int actor_pool_begin(pic_handle* h, ActorCall& k, const char* who) {
  if (k.features) return PIC_OK;
  const pic_actor* p = k.p;          // (`result`: the feature rows always exist, in the caller's memory or in the actor's block)
  return p->pool ? pool_begin(h, p->pool, k.x, k.v, p, "features_out", k.mem_kind, who, k.pool)
                 : pool_ln_begin(h, p->pool_ln, k.x, k.v, p, "features_out", k.mem_kind, who, k.pool);
}

// The block of a call, its inputs on the device and the argument block of its first step (the per-step pointers at row 0)
static int actor_begin(pic_handle* h, ActorCall& k, ActorArgs& a, const char* who) {
  const pic_actor* p = k.p;
  BlockDims d = block_dims(h);
  d.P = actor_param_count(p); d.per_env = p->per_env != 0;
  ActorCallShape s;
  s.nsteps = (size_t)k.nsteps; s.H = (size_t)p->width[0]; s.host = k.mem_kind == PIC_HOST; s.stepping = k.stepping;
  s.particles = !k.features; s.std = k.std; s.noise = k.noise;
  s.features_out = k.features_out; s.pre_out = k.pre_out; s.actions_out = k.actions_out; s.hist = k.hist;
  if (int rc = call_reserve<ActorCallViews>(h, h->pol, &h->pol_bytes, who, "the actor's device block", k,
                                            [&](Carver c, ActorCallViews& v) { return actor_parts(c, d, s, v); }))
    return rc;
  const size_t E = d.num_envs, T = s.nsteps, D = sizeof(double), nA = 2 * d.act_modes;
  a = ActorArgs{};
  HIPCHK(h, device_input(h, p->params, k.mem_kind, d.params() * D, k.d_params, &a.params));
  HIPCHK(h, device_input(h, k.std, k.mem_kind, nA * D, k.d_std, &a.std));
  HIPCHK(h, device_input(h, k.noise, k.mem_kind, T * E * nA * D, k.d_noise, &a.noise));
  HIPCHK(h, device_input(h, k.features, k.mem_kind, E * s.H * D, k.d_features, &a.features));
  a.feat_out = k.d_feat ? k.d_feat : k.features_out;       // (the block's rows, or the caller's device memory)
  a.pre_out = device_output(k.pre_out, k.mem_kind, k.d_pre_out);
  if (k.stepping) {
    a.act = k.d_act;
    a.act_out = k.mem_kind == PIC_DEVICE ? k.actions_out : nullptr;      // (host: the rows themselves are read back)
  } else {
    a.act = device_output(k.actions_out, k.mem_kind, k.d_act);
  }
  a.env_params = p->per_env ? (long long)d.P : 0;
  a.ln_eps = p->ln_eps; a.action_scale = p->action_scale; a.action_shift = p->action_shift;
  a.source = k.features ? kActorGiven : (p->pool ? kActorPool : kActorPoolLn);
  a.n_layers = p->n_layers;
  a.w0 = p->width[0]; a.w1 = p->width[1]; a.w2 = p->width[2]; a.w3 = p->width[3]; a.w4 = p->width[4]; a.w5 = p->width[5];
  a.w6 = p->width[6];
  a.layernorm = p->layernorm; a.activation = p->activation; a.squash = p->squash;
  return PIC_OK;
}

// the argument block of step s: every per-step row moved on by s steps
static ActorArgs actor_at(const ActorArgs& a0, size_t s, size_t E, size_t nA) {
  ActorArgs a = a0;
  const size_t rf = s * E * (size_t)a.w0, ra = s * E * nA;
  if (a.noise) a.noise += ra;
  if (a.feat_out) a.feat_out += rf;
  if (a.pre_out) a.pre_out += ra;
  if (a.act) a.act += ra;
  if (a.act_out) a.act_out += ra;
  return a;
}

// One evaluation: on particles the pool's max pass and pass (pool_forward's, both layers), then the kernel that finishes the sums
// and runs the head
static void actor_launch(pic_handle* h, const ActorCall& k, const ActorArgs& a) {
  const dim3 block(POOL_BLOCK);
  const PoolCall& c = k.pool;
  if (a.source != kActorGiven) {
    hipLaunchKernelGGL(pool_max_kernel, c.grid, block, 0, h->stream, c.a);
    if (c.shape.ln) hipLaunchKernelGGL(pool_ln_kernel, c.grid, block, 0, h->stream, c.a, c.n);
    else hipLaunchKernelGGL(pool_kernel, c.grid, block, 0, h->stream, c.a);
  }
  hipLaunchKernelGGL(actor_kernel, dim3(h->cfg.num_envs), block, 0, h->stream, a, c.a, c.n);
}

// the read-backs of a call in host memory and of the energies' record; one wait, if anything is read back.  `rc`: what the
// steps returned.  A failed call leaves the pool's sums unknown (pool_end's rule).
static int actor_finish(pic_handle* h, const ActorCall& k, const ActorArgs& a0, int rc, const char* who) {
  const size_t E = (size_t)h->cfg.num_envs, T = (size_t)k.nsteps, D = sizeof(double);
  const size_t H = (size_t)k.p->width[0], nA = 2 * (size_t)h->act_modes;
  hipError_t e = hipGetLastError();
  bool wait = false;
  if (k.mem_kind == PIC_HOST) {
    if (e == hipSuccess) e = device_result(h, k.features_out, a0.feat_out, T * E * H * D);
    if (e == hipSuccess) e = device_result(h, k.pre_out, a0.pre_out, T * E * nA * D);
    if (e == hipSuccess) e = device_result(h, k.actions_out, a0.act, T * E * nA * D);
    wait = k.features_out || k.pre_out || k.actions_out;
  }
  if (k.hist) {
    if (e == hipSuccess) e = hipMemcpyAsync(k.hist, k.d_hist, T * 3 * E * D, hipMemcpyDeviceToHost, h->stream);
    wait = true;
  }
  const int rf = hip_tail(h, e, wait, who);
  if ((rc || rf) && !k.features) h->pool_zero = 0;
  return rc ? rc : rf;
}

int pic_actor_eval(pic_handle* h, const pic_actor* p, const double* features, const void* x, const void* v, const double* noise,
                   const double* std, int mem_kind, double* features_out, double* pre_out, double* actions_out) {
  const char* who = "pic_actor_eval";
  if (!h) return PIC_EINVAL;
  if (const char* bad = actor_bad_args(p, mem_kind)) return fail(h, PIC_EINVAL, std::string(who) + ": " + bad);
  int rc = actor_actuator(h, p, who);
  if (rc) return rc;
  if (features && (x || v)) return fail(h, PIC_EINVAL, std::string(who) + ": features must not be given together with x or v");
  ActorCall k{{}, p, features, x, v, noise, std, mem_kind, 1, false, features_out, pre_out, actions_out, nullptr, {}};
  rc = actor_pool_begin(h, k, who);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  ActorArgs a;
  rc = actor_begin(h, k, a, who);
  if (rc) return rc;
  actor_launch(h, k, a);
  return actor_finish(h, k, a, PIC_OK, who);
}

int pic_step_actor(pic_handle* h, const pic_actor* p, const double* noise, const double* std, int mem_kind, int nsteps,
                   double* features_out, double* pre_out, double* actions_out, double* hist) {
  const char* who = "pic_step_actor";
  if (h && h->tape.on)
    return fail(h, PIC_ESTATE, "pic_step_actor: refused while a tape is open (there is no taped entry; a torch policy on the tape "
                               "is the route: its actions depend on the state)");
  int rc = step_prologue(h, nsteps, who, h ? actor_bad_args(p, mem_kind) : nullptr);
  if (rc) return rc;
  rc = actor_actuator(h, p, who);
  if (rc) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, who);
  if (rc) return rc;
  rc = pool_stored_check(h, who);        // (a call of no steps makes every check and enqueues nothing)
  if (rc || nsteps == 0) return rc;
  ActorCall k{{}, p, nullptr, nullptr, nullptr, noise, std, mem_kind, nsteps, true, features_out, pre_out, actions_out, hist, {}};
  rc = actor_pool_begin(h, k, who);      // (once per call: the block, its zeros and the pool's parameters serve every step)
  if (rc) return rc;
  ActorArgs a0;
  rc = actor_begin(h, k, a0, who);
  if (rc) return rc;
  // Step s: the actor on the particles step s-1 left, its features into row s of the features and its actions into row s of the
  // actions; then the step pic_step_actions(row s, 1) makes.  No action row and no feature row is written twice within a call,
  // so the launches of step s+1 cannot overtake a force evaluation of step s; the pool's sums are cleared by the kernel that
  // reads them, so every step finds them zero.
  const int E = h->cfg.num_envs;
  for (int s = 0; s < nsteps && rc == PIC_OK; ++s) {
    const ActorArgs a = actor_at(a0, (size_t)s, (size_t)E, 2 * (size_t)h->act_modes);
    actor_launch(h, k, a);
    sc.ctl.act = a.act;
    rc = advance(h, sc, 1, hist_at(h, k.d_hist, (size_t)s));
  }
  return actor_finish(h, k, a0, rc, who);      // (after a failed step too: what was enqueued is waited for)
}
