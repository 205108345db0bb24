// host_actor.h -- the host side of pic_actor_eval and pic_step_actor; kernel: pic_actor.h.
// Included by picstep.hip inside its extern "C" block, behind host_head.h (what a call shares with the MLP policy's: host_policy.h)
// and host_pool.h (the pool call that a call on particles begins: pool_begin, pool_ln_begin); the layout of its block is
// host_blocks.h's actor_parts, reserved through call_reserve on the handle's policy block.

// what is wrong with an actor whatever the actuator and the source of its features, or null: head_bad_shape and, at their places,
// the checks of its pool, its LayerNorm and its scales
static const char* actor_bad_args(const pic_actor* p, int mem_kind) {
  if (!p) return "null actor";
  return head_bad_shape(*p, mem_kind, kActorMaxLayers, [&](int slot) -> const char* {
    if (slot == kOwnBehindMemKind) {
      if (!p->pool == !p->pool_ln) return "exactly one of pool and pool_ln must be given";
      return p->pool ? pool_spec_error(p->pool) : pool_ln_spec_error(p->pool_ln);
    }
    if (slot == kOwnBehindWidths) {
      if (p->width[0] != (p->pool ? p->pool->hidden : p->pool_ln->hidden)) return "width[0] must be the pool's hidden";
      if (p->layernorm != 0 && p->layernorm != 1) return "layernorm must be 0 or 1";
    }
    if (slot == kOwnBehindFlags) {
      if (p->layernorm && !(std::isfinite(p->ln_eps) && p->ln_eps > 0.0)) return "ln_eps must be finite and > 0";
      if (!std::isfinite(p->action_scale) || !std::isfinite(p->action_shift)) return "action_scale and action_shift must be finite";
    }
    return nullptr;
  });
}

// One call's arguments on the views into the handle's policy block it works on (host_blocks.h: actor_parts)
struct ActorCall : ActorCallViews, HeadCall {
  const pic_actor* p;
  const double* features;
  const void *x, *v;
  PoolCall pool;             // the pool call of a call on particles (features == null)
};
static HeadRow<ActorArgs> actor_row(const pic_actor* p) { return {&ActorArgs::feat_out, (size_t)p->width[0]}; }

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
  d.P = head_param_count(p->width, p->n_layers, p->layernorm != 0); d.per_env = p->per_env != 0;
  ActorCallShape s;
  s.nsteps = (size_t)k.nsteps; s.H = (size_t)p->width[0]; s.host = k.mem_kind == PIC_HOST; s.stepping = k.stepping;
  s.particles = !k.features; s.std = k.std; s.noise = k.noise;
  s.features_out = k.row_out; s.pre_out = k.pre_out; s.actions_out = k.actions_out; s.hist = k.hist;
  if (int rc = call_reserve<ActorCallViews>(h, h->pol, &h->pol_bytes, who, "the actor's device block", k,
                                            [&](Carver c, ActorCallViews& v) { return actor_parts(c, d, s, v); }))
    return rc;
  a = ActorArgs{};
  if (int rc = head_stage(h, k, p->params, d, a)) return rc;
  HIPCHK(h, device_input(h, k.features, k.mem_kind, d.num_envs * s.H * sizeof(double), k.d_features, &a.features));
  a.feat_out = k.d_feat ? k.d_feat : k.row_out;            // (the block's rows, or the caller's device memory)
  a.ln_eps = p->ln_eps; a.action_scale = p->action_scale; a.action_shift = p->action_shift;
  a.source = k.features ? kActorGiven : (p->pool ? kActorPool : kActorPoolLn);
  a.n_layers = p->n_layers;
  a.w0 = p->width[0]; a.w1 = p->width[1]; a.w2 = p->width[2]; a.w3 = p->width[3]; a.w4 = p->width[4]; a.w5 = p->width[5];
  a.w6 = p->width[6];
  a.layernorm = p->layernorm; a.activation = p->activation; a.squash = p->squash;
  return PIC_OK;
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

// head_finish, and the actor's own rule: a failed call (rc: what the steps returned) leaves the pool's sums unknown (pool_end's)
static int actor_finish(pic_handle* h, const ActorCall& k, const ActorArgs& a0, int rc, const char* who) {
  const int rf = head_finish(h, k, a0, actor_row(k.p), who);
  if ((rc || rf) && !k.features) h->pool_zero = 0;
  return rc ? rc : rf;
}

int pic_actor_eval(pic_handle* h, const pic_actor* p, const double* features, const void* x, const void* v, const double* noise,
                   const double* std, int mem_kind, double* features_out, double* pre_out, double* actions_out) {
  const char* who = "pic_actor_eval";
  int rc = head_entry(h, p, actor_bad_args(p, mem_kind), who);
  if (rc) return rc;
  if (features && (x || v)) return fail(h, PIC_EINVAL, std::string(who) + ": features must not be given together with x or v");
  ActorCall k{{}, {noise, std, mem_kind, 1, false, features_out, pre_out, actions_out, nullptr}, p, features, x, v, {}};
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
  rc = head_actuator(h, p->width[p->n_layers], who);
  if (rc) return rc;
  StepControl sc;
  rc = actuator_control(h, sc, who);
  if (rc) return rc;
  rc = pool_stored_check(h, who);        // (a call of no steps makes every check and enqueues nothing)
  if (rc || nsteps == 0) return rc;
  ActorCall k{{}, {noise, std, mem_kind, nsteps, true, features_out, pre_out, actions_out, hist}, p, nullptr, nullptr, nullptr, {}};
  rc = actor_pool_begin(h, k, who);      // (once per call: the block, its zeros and the pool's parameters serve every step)
  if (rc) return rc;
  ActorArgs a0;
  rc = actor_begin(h, k, a0, who);
  if (rc) return rc;
  // (the actor's own row is the feature row; the pool's sums are cleared by the kernel that reads them, so every step finds
  // them zero)
  rc = head_steps(h, sc, a0, actor_row(p), nsteps, k.d_hist, [&](const ActorArgs& a) { actor_launch(h, k, a); });
  return actor_finish(h, k, a0, rc, who);
}
