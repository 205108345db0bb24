"""Differentiable rollouts for torch: the energy traces of a rollout as functions of its actions (or raw external fields), with
the gradient from the device's adjoint (pic_tape_backward) and forward-mode tangents from pic_tape_tangent (7f).

    KE, PE, PE_reward = rollout(env, actions)      # actions: float64 CUDA tensor [T, num_envs, 2*max_mode], requires_grad
    (PE_reward.sum() + lam * (actions ** 2).sum() * L / 4).backward()   # fills actions.grad
    with torch.autograd.forward_ad.dual_level():     # forward mode: the tangent of the traces along a direction du
        KE, PE, PE_reward = (fwAD.unpack_dual(o).tangent for o in rollout(env, fwAD.make_dual(actions, du)))

    KE, PE, PE_reward, modes = rollout_feedback(env, gain, T)   # gain: [num_envs, 2M, 2M] or [2M, 2M], requires_grad
    (PE_reward.sum() + (modes[..., 0] ** 2).sum()).backward()  # fills gain.grad through the closed loop

    KE, PE, PE_reward, actions, obs = rollout_policy(env, policy, T)   # policy: any torch callable, modes -> actions
    (PE_reward.sum() + lam * (actions ** 2).sum() * L / 4).backward()   # fills the policy's .grad through the closed loop (7e)

    KE, PE, PE_reward, actions, pre, obs = rollout_mlp(env, policy, params, T)   # policy: an MLPPolicy, params: its packed vector
    (PE_reward.sum() + lam * (actions ** 2).sum() * L / 4).backward()   # fills params.grad: one device call each way (7p)
    with fwAD.dual_level():                          # forward mode in params and std: one pic_tape_tangent_policy (7q)
        outs = rollout_mlp(env, policy, fwAD.make_dual(params, d_params), T)

rollout_policy(..., observe="moments") hands the policy the fluid moments on the mesh, [num_envs, 3, N_mesh], instead of the modes
(DESIGN.md 7k); the backward sets the policy's cotangent on them through pic_tape_moments_cot.

Every entry takes kl=dict(feq=..., vmin=..., vmax=...) (BatchedPIC.start_tape): the smoothed phase-space KL after every step,
[T, num_envs], is then appended as one more differentiable output, so that the reference's whole cost is:

    KE, PE, PE_reward, KL = rollout(env, actions, kl=dict(feq=feq, vmin=-6.0, vmax=6.0))
    (KL.sum() + PE_reward.sum()).backward()

In forward mode the KL output of rollout and rollout_ext carries its tangent like the energy traces (pic_tape_tangent_kl,
DESIGN.md 7j), so a directional derivative of the whole cost is one dual_level pass.

rollout and rollout_ext take moments=True: the fluid moments of the state every step left, [T, num_envs, 3, N_mesh], follow the
other outputs (KE, PE, PE_reward, then KL if asked, then the moments), differentiable in reverse (pic_tape_moments_cot) and in
forward mode (pic_tape_tangent_moments):

    KE, PE, PE_reward, mom = rollout(env, actions, moments=True)
    ((mom[:, :, 0] - target) ** 2).sum().backward()                 # a density-profile tracking cost

Each call opens a fresh tape on `env` (an open one is stopped first) and leaves it open for the backward; stop it with
`env.stop_tape()` before a reset.  A backward after the environment has moved on (a further step, another rollout, a reset)
raises PicError.
"""
import numpy as np
import torch

from .._abi import PicError


def _start(env, T, checkpoint_every, kl=None, moments=False):
    env.stop_tape()
    env.start_tape(T, checkpoint_every, kl=kl, moments=moments)
    env._tape_serial += 1
    return env._tape_serial


def _check_live(env, serial, steps, who):
    if env._tape_serial != serial or env.tape_stats()["steps"] != steps:
        raise PicError(f"{who}: the environment has moved on since this rollout (a further step, rollout or reset)")


class _Rollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, env, kind, checkpoint_every, kl=None, moments=False):
        if not (u.dtype == torch.float64 and u.dim() == 3 and u.shape[1] == env.num_envs):
            raise ValueError("the control must be a float64 tensor [T, num_envs, ...]")
        T = int(u.shape[0])
        serial = _start(env, T, checkpoint_every, kl, moments)
        host = np.ascontiguousarray(u.detach().cpu().numpy())
        if kind == "actions":
            ke, pe, per = env.step_actions_traj(host, history=True)
        else:
            ke, pe, per = env.step_ext_traj(host, history=True)
        ctx.env, ctx.kind, ctx.serial, ctx.steps, ctx.device, ctx.kl = env, kind, serial, T, u.device, kl is not None
        ctx.moments = bool(moments)
        outs = (ke, pe, per) + ((env.tape_kl(),) if kl is not None else ()) + ((env.tape_moments(),) if moments else ())
        return tuple(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=u.device) for a in outs)

    @staticmethod
    def backward(ctx, g_ke, g_pe, g_per, *g_extra):
        _check_live(ctx.env, ctx.serial, ctx.steps, "backward")
        g_extra = list(g_extra)
        g_kl = g_extra.pop(0) if ctx.kl else None
        g_mom = g_extra.pop(0) if ctx.moments else None
        out = ctx.env.backward(d_KE=g_ke, d_PE=g_pe, d_PE_reward=g_per, d_KL=g_kl, d_moments=g_mom)
        g = torch.as_tensor(out["actions" if ctx.kind == "actions" else "ext"])       # (NumPy out for CPU cotangents in)
        return g, None, None, None, None, None

    @staticmethod
    def jvp(ctx, u_t, env_t, kind_t, ce_t, kl_t=None, mom_t=None):
        """Forward mode (torch.autograd.forward_ad): the tangent of the energy traces along u_t, from pic_tape_tangent on the
        tape this rollout opened, of the KL trace of a rollout with kl=... from pic_tape_tangent_kl (7j) and of
        the moments' trace of one with moments=True from pic_tape_tangent_moments (7l)."""
        env = ctx.env
        _check_live(env, ctx.serial, ctx.steps, "jvp")
        zero = lambda *s: torch.zeros((ctx.steps, env.num_envs) + s, dtype=torch.float64, device=ctx.device)  # noqa: E731
        if u_t is None:
            return tuple(zero() for _ in range(4 if ctx.kl else 3)) + ((zero(3, env.N_mesh),) if ctx.moments else ())
        out = env.tangent(kl=ctx.kl, moments=ctx.moments, **{"d_actions" if ctx.kind == "actions" else "d_ext": u_t.detach()})
        keys = ("KE", "PE", "PE_reward") + (("KL",) if ctx.kl else ()) + (("moments",) if ctx.moments else ())
        return tuple(torch.as_tensor(out[k], dtype=torch.float64, device=ctx.device) for k in keys)


def rollout(env, actions, checkpoint_every=0, kl=None, moments=False):
    """T = actions.shape[0] steps of `env` (a BatchedPIC with an actuator) under actions [T, num_envs, 2*max_mode] through
    pic_step_actions_traj on a tape; returns KE, PE, PE_reward [T, num_envs] (float64, on actions' device), differentiable
    with respect to `actions`.  With kl=dict(feq=..., vmin=..., vmax=...) a fourth output follows: the smoothed KL after
    every step, [T, num_envs], differentiable too.  With moments=True one more output follows the others: the fluid moments of
    the state every step left, [T, num_envs, 3, N_mesh] (BatchedPIC.tape_moments), differentiable in both modes."""
    if env.max_mode == 0:
        raise PicError("rollout: the environment has no actuator (set_actuator)")
    return _Rollout.apply(actions, env, "actions", int(checkpoint_every), kl, bool(moments))


def rollout_ext(env, E_ext, checkpoint_every=0, kl=None, moments=False):
    """The same under raw external fields E_ext [T, num_envs, N_mesh] (pic_step_ext_traj)."""
    return _Rollout.apply(E_ext, env, "ext", int(checkpoint_every), kl, bool(moments))


class _RolloutFeedback(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gain, env, T, checkpoint_every, kl=None):
        E, n = env.num_envs, 2 * env.max_mode
        if not (gain.dtype == torch.float64 and tuple(gain.shape) in ((E, n, n), (n, n))):
            raise ValueError(f"the gain must be a float64 tensor [{E}, {n}, {n}] or [{n}, {n}]")
        serial = _start(env, T, checkpoint_every, kl)
        g = gain.detach()
        if not g.is_cuda:
            g = g.numpy()
        out = env.step_feedback_gain(g, T, modes=True, history=True)
        ctx.env, ctx.serial, ctx.steps, ctx.shared, ctx.kl = env, serial, T, gain.dim() == 2, kl is not None
        ctx.device = gain.device
        outs = [out[k] for k in ("KE", "PE", "PE_reward", "modes")] + ([env.tape_kl()] if kl is not None else [])
        return tuple(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=gain.device) for a in outs)

    @staticmethod
    def backward(ctx, g_ke, g_pe, g_per, g_modes, g_kl=None):
        _check_live(ctx.env, ctx.serial, ctx.steps, "backward")
        out = ctx.env.backward(d_KE=g_ke, d_PE=g_pe, d_PE_reward=g_per, d_modes=g_modes, d_KL=g_kl if ctx.kl else None)
        g = torch.as_tensor(out["gain"])             # (NumPy out for CPU cotangents in)
        return (g.sum(0) if ctx.shared else g), None, None, None, None

    @staticmethod
    def jvp(ctx, gain_t, env_t, T_t, ce_t, kl_t=None):
        """Forward mode (torch.autograd.forward_ad): the tangents of the traces and of the law's modes along gain_t, from
        pic_tape_tangent_feedback on the tape this rollout opened.  The KL's tangent through the closed loop is
        not built."""
        env = ctx.env
        _check_live(env, ctx.serial, ctx.steps, "jvp")
        if ctx.kl:
            raise NotImplementedError("rollout_feedback: forward mode of the KL through the gain law is not built (DESIGN.md 7n)")
        E, n = env.num_envs, 2 * env.max_mode
        if gain_t is None:
            z = lambda *s: torch.zeros((ctx.steps, E) + s, dtype=torch.float64, device=ctx.device)  # noqa: E731
            return z(), z(), z(), z(n)
        g = gain_t.detach().to(torch.float64)
        if ctx.shared:
            g = g.expand(E, n, n)
        g = g.contiguous()
        out = env.tangent_feedback(d_gain=g if g.is_cuda else g.numpy())
        return tuple(torch.as_tensor(np.ascontiguousarray(out[k]) if isinstance(out[k], np.ndarray) else out[k],
                                     dtype=torch.float64, device=ctx.device) for k in ("KE", "PE", "PE_reward", "modes"))


def rollout_feedback(env, gain, T, checkpoint_every=0, kl=None):
    """T steps of `env` (a BatchedPIC with an actuator) under the closed-loop gain law a_t = G m_t (step_feedback_gain) on a
    tape; returns KE, PE, PE_reward [T, num_envs] and the modes m_t [T, num_envs, 2*max_mode] the law read, differentiable with
    respect to `gain` (float64, [num_envs, 2M, 2M], or [2M, 2M] shared by every environment: its gradient is the sum over
    them).  Cotangents on `modes` reach the plasma through d_modes, so spectral losses such as sum |E_1|^2 work too.  With kl=...
    the smoothed KL after every step, [T, num_envs], follows as a fifth differentiable output."""
    if env.max_mode == 0:
        raise PicError("rollout_feedback: the environment has no actuator (set_actuator)")
    return _RolloutFeedback.apply(gain, env, int(T), int(checkpoint_every), kl)


class _PolicyWalk:
    """What the steps of one rollout_policy share: the environment, the tape's identity, and the reverse walk their backwards
    advance together (step T-1 first, the start last)."""

    def __init__(self, env, T, observe, obs_modes, serial, kl=False):
        self.env, self.T, self.observe, self.obs_modes, self.serial, self.kl = env, T, observe, obs_modes, serial, kl
        self.walk, self.next = None, -1

    def reverse_to(self, t):
        """Make step t the next one to reverse: open a walk if none is running, and reverse the steps after t that no
        cotangent reached (no output of theirs was used) with zero cotangents."""
        env = self.env
        if self.walk is None:
            _check_live(env, self.serial, self.T, "backward")
            self.walk, self.next = env.walk(self.obs_modes, on_device=True), self.T - 1
        if self.next < t:
            raise PicError(f"backward: step {t} reached after step {self.next + 1} was reversed (out of order)")
        while self.next > t:
            self.walk.step()
            self.next -= 1

    def cot(self, g_obs):
        """Cotangents of an observation -> walk arguments."""
        if self.observe == "modes":
            return {"d_modes": g_obs[0]}
        if self.observe == "moments":
            return {"d_moments": g_obs[0]}
        return {"d_x": g_obs[0], "d_v": g_obs[1]}


def _observe(env, observe, obs_modes):
    if observe == "modes":
        return (env.modes_torch(obs_modes),)
    if observe == "moments":
        return (env.moments_torch(),)
    v = env._ordered_views()
    return tuple(v[k].clone(memory_format=torch.contiguous_format) for k in ("x", "v"))


class _PolicyStart(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, pw):
        ctx.set_materialize_grads(False)
        ctx.pw = pw
        return (anchor.new_zeros(0),) + _observe(pw.env, pw.observe, pw.obs_modes)

    @staticmethod
    def backward(ctx, g_token, *g_obs):
        pw = ctx.pw
        pw.reverse_to(-1)
        walk, pw.walk = pw.walk, None
        walk.end(**{k + "0": v for k, v in pw.cot(g_obs).items()})
        return None, None


class _PolicyStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, token, action, pw, t):
        ctx.set_materialize_grads(False)
        ctx.pw, ctx.t = pw, t
        env = pw.env
        env.step_actions_torch(action.detach().contiguous())
        en = env.energy_views_torch()
        energies = tuple(en[k].clone() for k in ("KE", "PE", "PE_reward"))
        if pw.kl:                                    # the KL of this step: its row of the tape's trace
            energies += (env.tape_kl(on_device=True)[t].clone(),)
        return (token.new_zeros(0),) + energies + _observe(env, pw.observe, pw.obs_modes)

    @staticmethod
    def backward(ctx, g_token, g_ke, g_pe, g_per, *g_obs):
        pw, t = ctx.pw, ctx.t
        pw.reverse_to(t)
        kw = {}
        if pw.kl:
            kw["d_kl"], g_obs = g_obs[0], g_obs[1:]
        d_en = None
        if any(g is not None for g in (g_ke, g_pe, g_per)):
            ref = next(g for g in (g_ke, g_pe, g_per) if g is not None)
            d_en = torch.stack([g if g is not None else torch.zeros_like(ref) for g in (g_ke, g_pe, g_per)])
        _, _, g_act = pw.walk.step(d_energies=d_en, **kw, **pw.cot(g_obs))
        pw.next -= 1
        return g_token.new_zeros(0) if g_token is not None else None, g_act, None, None


def rollout_policy(env, policy, T, observe="modes", obs_modes=None, checkpoint_every=0, kl=None):
    """T steps of `env` (a BatchedPIC with an actuator, on the GPU) in closed loop under a torch policy: at every step the
    observation o_t goes through `policy(o_t)` to the actions a_t [num_envs, 2*max_mode] (any float dtype: cast to float64), which
    step_actions_torch applies.  observe="modes": o_t = the modes of the field, float64 [num_envs, 2*M_o] (Re E_1..E_Mo then
    Im, obs_modes M_o defaulting to max_mode); observe="state": o_t = (x, v), a tuple of float64 copies [num_envs, N] of the
    particles (torch.cat(o_t, 1) is the reference actor's input); observe="moments": o_t = the fluid moments on the mesh, float64
    [num_envs, 3, N_mesh] (BatchedPIC.moments: density, momentum density, twice the kinetic-energy density; the policy derives
    u = m1 / m0 and T = m2 / m0 - u^2 itself, where autograd sees it).
    Runs on a fresh tape; returns KE, PE, PE_reward [T, num_envs], actions [T, num_envs, 2*max_mode] and the observations
    o_0..o_T (a list of T + 1), all differentiable with respect to the policy's parameters (and whatever else it closes over):
    the backward walks the tape step by step (pic_tape_walk_*) and puts the policy's own vector-Jacobian product
    between two reverse steps.  With env.use_torch_stream() no step synchronises the host.  With kl=... the smoothed KL after
    every step, [T, num_envs], follows as a sixth differentiable output (reading each step's value waits for the step)."""
    if env.max_mode == 0:
        raise PicError("rollout_policy: the environment has no actuator (set_actuator)")
    if observe not in ("modes", "state", "moments"):
        raise ValueError('observe must be "modes", "state" or "moments"')
    T = int(T)
    if T < 1:
        raise ValueError("need T >= 1")
    mo = int(obs_modes) if obs_modes is not None else env.max_mode
    if not 1 <= mo < env.N_mesh:
        raise ValueError("need 1 <= obs_modes < N_mesh")
    serial = _start(env, T, int(checkpoint_every), kl)
    pw = _PolicyWalk(env, T, observe, mo, serial, kl is not None)
    anchor = torch.zeros(0, dtype=torch.float64, device=f"cuda:{env.device}", requires_grad=True)
    out = _PolicyStart.apply(anchor, pw)
    token, o = out[0], (tuple(out[1:]) if observe == "state" else out[1])
    obs = [o]
    ke, pe, per, acts, kls = [], [], [], [], []
    n = 2 * env.max_mode
    k0 = 5 if kl is not None else 4                  # where a step's observation starts in its outputs
    for t in range(T):
        a = policy(o).to(torch.float64)
        if tuple(a.shape) != (env.num_envs, n):
            raise ValueError(f"the policy must return actions [{env.num_envs}, {n}], not {tuple(a.shape)}")
        out = _PolicyStep.apply(token, a, pw, t)
        token, o = out[0], (tuple(out[k0:]) if observe == "state" else out[k0])
        ke.append(out[1])
        pe.append(out[2])
        per.append(out[3])
        if kl is not None:
            kls.append(out[4])
        acts.append(a)
        obs.append(o)
    res = (torch.stack(ke), torch.stack(pe), torch.stack(per), torch.stack(acts), obs)
    return res + ((torch.stack(kls),) if kl is not None else ())


class _RolloutMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, std, env, policy, T, noise, checkpoint_every, kl=None):
        ctx.set_materialize_grads(False)
        serial = _start(env, T, checkpoint_every, kl)
        r = env.tape_step_policy(policy.with_params(params.detach().contiguous()), T, noise=noise,
                                 std=None if std is None else std.detach(), history=True, on_device=True)
        ctx.env, ctx.serial, ctx.steps, ctx.kl, ctx.squash = env, serial, T, kl is not None, policy.squash
        ctx.noise, ctx.has_std = noise, std is not None
        dev = params.device
        energies = tuple(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev) for a in (r.KE, r.PE, r.PE_reward))
        return energies + (r.actions, r.pre, r.obs) + ((env.tape_kl(on_device=True),) if kl is not None else ())

    @staticmethod
    def backward(ctx, g_ke, g_pe, g_per, g_act, g_pre, g_obs, g_kl=None):
        env = ctx.env
        _check_live(env, ctx.serial, ctx.steps, "backward")
        if g_pre is not None:
            if ctx.squash:
                raise NotImplementedError("rollout_mlp: a cotangent on `pre` of a squashed policy is not built (use `actions`)")
            g_act = g_pre if g_act is None else g_act + g_pre      # (a = u without squash)
        dev = f"cuda:{env.device}"
        on = lambda g: None if g is None else g.to(dev)  # noqa: E731
        out = env.backward_policy(d_KE=on(g_ke), d_PE=on(g_pe), d_PE_reward=on(g_per), d_actions=on(g_act), d_obs=on(g_obs),
                                  d_KL=on(g_kl) if ctx.kl else None)
        g_params = torch.as_tensor(out["params"], dtype=torch.float64, device=dev)
        g_std = None
        if ctx.has_std and ctx.noise is not None:
            eps = torch.as_tensor(ctx.noise, dtype=torch.float64, device=dev).reshape(ctx.steps, env.num_envs, -1)
            g_std = (torch.as_tensor(out["pre"], dtype=torch.float64, device=dev) * eps).sum((0, 1))
        return g_params, g_std, None, None, None, None, None, None

    @staticmethod
    def jvp(ctx, params_t, std_t, env_t, policy_t, T_t, noise_t, ce_t, kl_t=None):
        """Forward mode (torch.autograd.forward_ad): the tangents of the traces, the actions, pre and obs along (params_t, std_t),
        from one pic_tape_tangent_policy with K = 1 on the tape this rollout opened.  The KL's tangent through the
        closed loop is not built."""
        env = ctx.env
        _check_live(env, ctx.serial, ctx.steps, "jvp")
        if ctx.kl:
            raise NotImplementedError("rollout_mlp: forward mode of the KL through the policy is not built (DESIGN.md 7q)")
        dev = f"cuda:{env.device}"
        on = lambda a: None if a is None else a.detach().to(dev, torch.float64).contiguous()  # noqa: E731
        d_std = on(std_t) if ctx.has_std and ctx.noise is not None else None
        out = env.tangent_policy(d_params=on(params_t), d_std=d_std, noise=ctx.noise if d_std is not None else None, on_device=True)
        return tuple(out[k].contiguous() for k in ("dKE", "dPE", "dPE_reward", "d_actions", "d_pre", "d_obs"))


def rollout_mlp(env, policy, params, T, noise=None, std=None, checkpoint_every=0, kl=None):
    """T steps of `env` (a BatchedPIC with an actuator, on the GPU) in closed loop under the MLP `policy`
    (control.policy.MLPPolicy: its shape, scales and squash) with the packed parameters `params`, a float64 CUDA tensor [P] or
    [num_envs, P] (one vector per environment): ONE autograd function for the whole rollout.  The forward is
    start_tape plus one tape_step_policy, the backward one backward_policy: no step returns to Python in either direction.
    noise: eps [T, num_envs, 2M] or None; std: a float64 tensor [2M] or None.  Returns KE, PE, PE_reward [T, num_envs], actions
    and pre [T, num_envs, 2M], obs [T, num_envs, 2 M_o] (obs[t] is what step t's policy read), and with kl=... the smoothed KL
    after every step; all differentiable with respect to `params` and `std`.  `MLPPolicy.unpack_grad` gives params.grad the
    layers' shapes.  Under torch.autograd.forward_ad the outputs carry their tangents along (params, std) from one
    BatchedPIC.tangent_policy; with kl=... forward mode raises NotImplementedError."""
    if env.max_mode == 0:
        raise PicError("rollout_mlp: the environment has no actuator (set_actuator)")
    T = int(T)
    if T < 1:
        raise ValueError("need T >= 1")
    if not (torch.is_tensor(params) and params.is_cuda and params.dtype == torch.float64 and params.dim() in (1, 2)):
        raise ValueError("params must be a float64 CUDA tensor [P] or [num_envs, P]")
    if std is not None and not torch.is_tensor(std):
        raise ValueError("std must be a tensor or None")
    from ..control.policy import MLPPolicy
    shape = MLPPolicy(policy.widths, policy.activation, params.detach(), policy.obs_modes, policy.squash, policy.action_scale,
                      policy.obs_scale, per_env=params.dim() == 2)
    return _RolloutMLP.apply(params, std, env, shape, T, noise, int(checkpoint_every), kl)


def _policy_jvp(fn, params, o, d_params, d_o):
    """The Jacobian-vector product of fn(params, o) along (d_params, d_o): torch.func.jvp where this torch has it, else
    torch.autograd.forward_ad."""
    if hasattr(torch, "func") and hasattr(torch.func, "jvp"):
        return torch.func.jvp(fn, (params, o), (d_params, d_o))[1]
    import torch.autograd.forward_ad as fwAD
    with fwAD.dual_level():
        dual = lambda a, t: fwAD.make_dual(a, t)  # noqa: E731
        p = {k: dual(a, d_params[k]) for k, a in params.items()}
        od = tuple(dual(a, t) for a, t in zip(o, d_o)) if isinstance(o, tuple) else dual(o, d_o)
        t = fwAD.unpack_dual(fn(p, od)).tangent
        return torch.zeros_like(fn(params, o)) if t is None else t


def rollout_policy_jvp(env, fn, params, d_params, T, observe="modes", obs_modes=None, d_x0=None, d_v0=None, checkpoint_every=0):
    """Forward mode through a closed loop under a torch policy written fn(params, o) -> actions [num_envs, 2*max_mode]
    (DESIGN.md 7n): the directional derivatives of the traces along K <= 8 directions at once.  params: a dict of tensors on the
    environment's device; d_params: a list of K dicts of tangents (missing names = 0); d_x0, d_v0 [K, num_envs, N]: tangents of
    the starting particles (None = 0).  observe="modes" (o_t = the modes [num_envs, 2*M_o]) or "state" (o_t = (x, v)) as in
    rollout_policy; "moments" is not built in forward mode.  Runs the loop on a fresh tape without grad, then walks it forward
    (pic_tape_tangent_walk_*): per step and direction d_a_t = the JVP of fn at (params, o_t) along (d_params[k], d_o_t[k]) goes
    in as the step's d_actions, and the step's tangent of the observation is d_o_{t+1}.  Returns a dict: the primal "KE", "PE",
    "PE_reward" [T, num_envs], "actions" [T, num_envs, 2M], "obs" (o_0..o_T) and the tangents "dKE", "dPE", "dPE_reward"
    [K, T, num_envs], "d_actions" [K, T, num_envs, 2M], "d_x", "d_v" [K, num_envs, N] (final particles)."""
    if env.max_mode == 0:
        raise PicError("rollout_policy_jvp: the environment has no actuator (set_actuator)")
    if observe == "moments":
        raise ValueError('rollout_policy_jvp: observe="moments" is not built in forward mode (DESIGN.md 7n)')
    if observe not in ("modes", "state"):
        raise ValueError('observe must be "modes" or "state"')
    T, K = int(T), len(d_params)
    if T < 1:
        raise ValueError("need T >= 1")
    if not 1 <= K <= 8:
        raise ValueError("need 1 <= len(d_params) <= 8")
    mo = int(obs_modes) if obs_modes is not None else env.max_mode
    if not 1 <= mo < env.N_mesh:
        raise ValueError("need 1 <= obs_modes < N_mesh")
    unknown = sorted({k for d in d_params for k in d} - set(params))
    if unknown:
        raise ValueError(f"d_params names unknown parameters: {unknown}")
    E, N, n = env.num_envs, env.N, 2 * env.max_mode
    dev = f"cuda:{env.device}"
    _start(env, T, int(checkpoint_every))
    ke, pe, per, acts = [], [], [], []
    with torch.no_grad():
        o = _observe(env, observe, mo)
        o = o if observe == "state" else o[0]
        obs = [o]
        for _ in range(T):
            a = fn(params, o).to(torch.float64)
            if tuple(a.shape) != (E, n):
                raise ValueError(f"the policy must return actions [{E}, {n}], not {tuple(a.shape)}")
            env.step_actions_torch(a.contiguous())
            en = env.energy_views_torch()
            ke.append(en["KE"].clone()), pe.append(en["PE"].clone()), per.append(en["PE_reward"].clone())
            acts.append(a)
            o = _observe(env, observe, mo)
            o = o if observe == "state" else o[0]
            obs.append(o)
    full = [{k: (torch.as_tensor(d[k], dtype=p.dtype, device=p.device) if k in d else torch.zeros_like(p)) for k, p in params.items()}
            for d in d_params]
    t64 = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64, device=dev).reshape(K, E, N)  # noqa: E731
    dx0, dv0 = t64(d_x0), t64(d_v0)
    walk = env.tangent_walk(K=K, obs_modes=mo if observe == "modes" else 0, d_x0=dx0, d_v0=dv0, on_device=True)
    zeros = torch.zeros((K, E, N), dtype=torch.float64, device=dev)
    d_o = walk.d_modes0 if observe == "modes" else (dx0 if dx0 is not None else zeros, dv0 if dv0 is not None else zeros)
    dke, dpe, dper, dacts = [], [], [], []
    for t in range(T):
        rows = [d_o[k] if observe == "modes" else (d_o[0][k], d_o[1][k]) for k in range(K)]
        da = torch.stack([_policy_jvp(fn, params, obs[t], full[k], rows[k]).to(torch.float64) for k in range(K)])
        r = walk.step(d_actions=da, state=observe == "state")
        dke.append(r["KE"]), dpe.append(r["PE"]), dper.append(r["PE_reward"]), dacts.append(r["actions"])
        d_o = r["modes"] if observe == "modes" else (r["x"], r["v"])
    d_x, d_v = walk.end()
    return {"KE": torch.stack(ke), "PE": torch.stack(pe), "PE_reward": torch.stack(per), "actions": torch.stack(acts), "obs": obs,
            "dKE": torch.stack(dke, 1), "dPE": torch.stack(dpe, 1), "dPE_reward": torch.stack(dper, 1),
            "d_actions": torch.stack(dacts, 1), "d_x": d_x, "d_v": d_v}
