"""Batched rollout environments: `num_envs` independent PIC systems stepped by one
libpicstep handle on one MI355X (BASELINE configs 2-5).  Nothing couples the
environments inside a step; across GPUs they are sharded rank-wise
(`.sharded.ShardedPIC`), never split.
"""
from typing import Optional

import numpy as np

from .. import _abi
from ._arrays import Mem
from .record import Record, recorder_args, recording_session


class _DeviceView:
    """Minimal __cuda_array_interface__ carrier so torch can alias library-owned memory."""

    def __init__(self, ptr, shape, typestr, strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": strides}


class BatchedPIC:
    def __init__(self, num_envs: int, N: int, N_mesh: int, n0: float = 1.0, L: float = 50.0, dt: float = 0.1,
                 gamma: float = 5.0, interpol: str = "CIC", device: int = 0, dtype="float64", accum_dtype=None,
                 blocks_per_env: int = 0, verbose: bool = False, env_index_base: int = 0, position_dtype=None,
                 placement: str = "auto", placement_ms: int = 0, integrator="symplectic_4th_order", readonly_c: str = "auto"):
        self.num_envs, self.N, self.N_mesh = int(num_envs), int(N), int(N_mesh)
        self.n0, self.L, self.gamma, self.interpol = n0, L, gamma, interpol
        self.dx = L / N_mesh
        # CFL clamp of PIC.initialize (src/env/pic.py:71-73)
        self.dt = dt
        if self.dt > 2 / np.sqrt(self.N / self.L):
            self.dt = 2 / np.sqrt(self.N / self.L)
            if verbose:
                print("CFL condtion invalid: change dt = {:.4f}".format(self.dt))
        self.device = device
        self.dtype = np.dtype(dtype)
        self._h = _abi.Handle(self.N, self.N_mesh, self.num_envs, L, n0, self.dt, gamma, self.dtype, accum_dtype,
                              interpol, device, blocks_per_env, env_index_base, position_dtype, placement, placement_ms,
                              integrator, readonly_c)
        self.integrator = _abi.INTEGRATOR_NAMES[_abi.integrator_id(integrator)]
        # what another BatchedPIC of the same physics is made with (env.plan.MPPI builds its samples from it)
        self._like = dict(N=self.N, N_mesh=self.N_mesh, n0=n0, L=L, dt=self.dt, gamma=gamma, interpol=interpol, device=device,
                          dtype=self.dtype, accum_dtype=accum_dtype, position_dtype=position_dtype, integrator=self.integrator)
        self._actuator = None
        self.fixed_positions = self._h.fixed_positions
        self.max_mode = 0                    # (no actuator yet: set_actuator)
        self._torch_stream = None            # (the handle runs on its own stream: use_torch_stream)
        self._tape_kl = False                # (the open tape records the smoothed KL)
        self._tape_moments = False           # (the open tape has held cotangents on the moments)
        self._tape_mom_trace = False         # (the open tape records the moments of every step)
        self._tape_policy = None             # (obs width, P, per_env) of the open tape's policy steps
        self._tape_serial = self._walk_serial = 0       # (the tape env.grad opened last, the walk in progress)

    # reset(x0, v0): x0, v0 are [num_envs, N] with any velocity perturbation already applied
    def reset(self, x0, v0):
        self._h.reset(x0, v0)

    def reset_sampled(self, kind: str = "bump-on-tail", a: float = 0.2, v0: float = 3.0, sigma: float = 1.0,
                      A: float = 0.1, n_mode: int = 2, seed: int = 0):
        """`reinit()` for every environment with the sample drawn on the device: the distributions of the
        reference's TwoStream / BumpOnTail (same particle ordering), velocity perturbation included.  A new
        `seed` gives a new ensemble; environment e always differs from environment e'.  Not NumPy's RNG
        stream -- use `reset(x0, v0)` with the host samplers when the reference's exact particles are wanted.
        Velocities before the perturbation lie in [-10, 10], the support of the reference's proposal.  Raises PicError
        for sigma < 1/sqrt(2 pi): there the reference accepts with u < pdf(v) > 1 somewhere, so its density is the
        clipped min(pdf, 1), which the device does not draw; use the host samplers (`env.dist`) and `reset` instead."""
        self._h.reset_sampled(kind, a, v0, sigma, A, n_mode, seed)

    def reset_device(self, x_ptr, v_ptr):
        self._h.reset_device(x_ptr, v_ptr)

    def step(self, E_external: Optional[np.ndarray] = None, nsteps: int = 1):
        """nsteps x update_state for every environment; asynchronous (call sync() or a getter)."""
        self._h.step(E_external, nsteps)

    def simulate(self, nsteps: int, E_external: Optional[np.ndarray] = None):
        """The energy traces of PIC.simulate (pic.py:175-223) for every environment, without its particle
        snapshots: -> (E, PE), each [nsteps + 1, num_envs], entry 0 = the state before the first step, as the
        reference records it.  The steps run back to back on the device; one read-back at the end."""
        ke0, pe0, _ = self.energies()
        ke, pe, _ = self._h.step_history(E_external, nsteps)
        return np.concatenate([(ke0 + pe0)[None], ke + pe]), np.concatenate([pe0[None], pe])

    def simulate_snapshots(self, nsteps: int, E_external: Optional[np.ndarray] = None):
        """PIC.simulate's snapshots for every environment: (x, v) after each step, each [nsteps, num_envs, N] of the
        particle dtype, and (KE, PE, PE_reward) [nsteps, num_envs]; one read-back for all steps (mind the size:
        nsteps x 2 x num_envs x N values are held on the device until the end of the call)."""
        return self._h.step_snapshots(E_external, nsteps)

    def step_history(self, E_external: Optional[np.ndarray] = None, nsteps: int = 1):
        """nsteps x update_state; -> (KE, PE, PE_reward) after every step, each [nsteps, num_envs]."""
        return self._h.step_history(E_external, nsteps)

    def step_device(self, E_ext_ptr=0, nsteps: int = 1):
        self._h.step_device(E_ext_ptr, nsteps)

    def sync(self):
        self._h.sync()

    def get_state(self):
        """[num_envs, 2N] float64: per environment the reference's get_state() column, flattened."""
        x, v = self._h.particles()
        return np.concatenate([x, v], axis=1, dtype=np.float64)

    def particles(self):
        return self._h.particles()

    def fields(self):
        return self._h.fields()

    def energies(self):
        """(KE, PE, PE_reward), each [num_envs]."""
        return self._h.energies()

    def rewards(self):
        """max(1 - PE_reward, 0) per environment (reward.py:72 with r_pe_n = 1)."""
        return np.maximum(1.0 - self._h.energies()[2], 0.0)

    def gather_E(self):
        return self._h.gather_E()

    def eval_field(self, x, E_ext=None):
        return self._h.eval_field(x, E_ext)

    # -- control loop on the device ---------------------------------------
    def set_actuator(self, actuator):
        """Upload an `E_field`'s basis tables (its linspace mesh included) for `step_actions`."""
        self._h.set_actuator(actuator.basis_cos, actuator.basis_sin)
        self.max_mode = actuator.max_mode
        self._actuator = actuator

    def step_actions(self, actions, nsteps: int = 1):
        """actions [num_envs, 2*max_mode] (cos coefficients, then sin): E_ext is built on the device
        (actuator.py:54-63) and held for `nsteps` steps."""
        self._h.step_actions(actions, nsteps)

    def step_observe(self, E_external: Optional[np.ndarray] = None, actions: Optional[np.ndarray] = None, nsteps: int = 1):
        """One iteration of a Gym-style loop for every environment in ONE call with ONE synchronisation (pic_step_observe;
        ddpg.py:421-468: update_state -> get_state -> reward): nsteps steps under E_external [num_envs, Ng] or actions
        [num_envs, 2*max_mode] (or neither) -> (state [num_envs, 2N] float64, (KE, PE, PE_reward) each [num_envs])."""
        x, v, ke, pe, per = self._h.step_observe(E_external, actions, nsteps)
        return np.concatenate([x, v], axis=1, dtype=np.float64), (ke, pe, per)

    def step_actions_device(self, actions_ptr, nsteps: int = 1):
        self._h.step_actions_device(actions_ptr, nsteps)

    def step_actions_traj(self, actions, history: bool = False):
        """A rollout with a new action every step in ONE call (pic_step_actions_traj): actions
        [nsteps, num_envs, 2*max_mode]; step s runs under actions[s] -- the inner loop of the trainers
        (src/control/rl/ddpg.py:421-468) once the actions are known.  history=True -> (KE, PE, PE_reward), each
        [nsteps, num_envs], after every step; otherwise asynchronous."""
        return self._h.step_actions_traj(actions, history)

    def step_actions_traj_torch(self, actions):
        """The same from a float64 CUDA tensor [nsteps, num_envs, 2*max_mode], consumed in stream order."""
        if not (actions.is_cuda and actions.dtype.is_floating_point and actions.element_size() == 8 and actions.is_contiguous()
                and actions.dim() == 3 and tuple(actions.shape[1:]) == (self.num_envs, 2 * self.max_mode)):
            raise ValueError("actions must be a contiguous float64 CUDA tensor [nsteps, num_envs, 2*max_mode]")
        shared = self._torch_stream is not None
        if not shared:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._h.step_actions_traj_device(actions.data_ptr(), int(actions.shape[0]))
        if not shared:
            self._h.sync()

    def step_ext_traj(self, E_ext_traj, history: bool = False, snapshots: bool = False):
        """PIC.simulate's E_external_traj (pic.py:175-223) for every environment in one call: E_ext_traj
        [nsteps, num_envs, N_mesh]; step s runs under E_ext_traj[s]."""
        return self._h.step_ext_traj(E_ext_traj, history, snapshots)

    def step_feedback(self, nsteps: int, actions: bool = False, history: bool = False):
        """nsteps iterations of run_feedback.py:130-168's loop body on the device (pic_step_feedback): before each step the
        actuator coefficients become (-Re E_k, +Im E_k), k = 1..max_mode, of the current E_mesh.  Bit for bit the host loop
        `step_actions(feedback_actions(max_mode))`.  Returns a dict with "actions" [nsteps, num_envs, 2*max_mode] and / or
        "KE", "PE", "PE_reward" [nsteps, num_envs] as asked for (None, and asynchronous, with neither)."""
        return self._h.step_feedback(nsteps, actions, history)

    def step_feedback_gain(self, gain, nsteps: int, actions: bool = False, modes: bool = False, history: bool = False):
        """nsteps of the linear law a = G m on the device (pic_step_feedback_gain): before each step
        m = (Re E_1..Re E_M, Im E_1..Im E_M) of the current E_mesh (M = max_mode) and a[i] = sum_k G[i][k] m[k] over the non-zero
        G[i][k] in ascending k.  gain: NumPy or a float64 CUDA tensor, [num_envs, 2M, 2M] or [2M, 2M] for every environment;
        G0 = diag(-1 x M, +1 x M) is step_feedback bit for bit.  Allowed while a tape is open (the steps are differentiable
        through the law: backward returns "modes" and "gain").  Returns a dict with "actions", "modes" [nsteps, num_envs, 2M]
        and / or "KE", "PE", "PE_reward" [nsteps, num_envs] as asked for (None, and asynchronous, with none of them)."""
        E, n = self.num_envs, 2 * self.max_mode
        if hasattr(gain, "is_cuda") and gain.is_cuda:
            import torch
            if gain.dtype != torch.float64:
                raise ValueError("gain must be float64")
            g = gain.reshape(1, n, n).expand(E, n, n) if gain.dim() == 2 else gain
            if tuple(g.shape) != (E, n, n):
                raise ValueError(f"gain must be [{E}, {n}, {n}] or [{n}, {n}]")
            g = g.contiguous()
            shared = self._torch_stream is not None
            if not shared:
                torch.cuda.current_stream(self.device).synchronize()
            out = self._h.step_feedback_gain(None, nsteps, actions, modes, history, device_ptr=g.data_ptr())
            if not shared and out is None:
                self._h.sync()           # (g, a temporary, must outlive the steps that read it)
            return out
        g = np.asarray(gain, dtype=np.float64)
        if g.shape == (n, n):
            g = np.broadcast_to(g, (E, n, n))
        return self._h.step_feedback_gain(np.ascontiguousarray(g), nsteps, actions, modes, history)

    # -- closed loops under an MLP policy on the device (pic_policy_eval, pic_step_policy) ------------------
    def _policy_call(self, policy, T, obs, noise, std, on_device):
        """The memory, the struct and the arrays of one policy call: inputs as float64 arrays of that memory, fresh outputs."""
        E, nO, nA = self.num_envs, 2 * policy.obs_modes, 2 * self.max_mode
        mem = Mem.of(self, policy.params, obs, noise, std, force_device=on_device)
        spec, keep = policy.spec(mem, E)
        lead = () if T is None else (T,)
        obs = mem.f64(obs, (E, nO))
        noise = mem.f64(noise, lead + (E, nA))
        std = mem.f64(std, (nA,))
        outs = mem.empty(lead + (E, nO)), mem.empty(lead + (E, nA)), mem.empty(lead + (E, nA))
        return mem, spec, keep, obs, noise, std, outs

    def policy_eval(self, policy, obs=None, noise=None, std=None, on_device: bool = False):
        """`policy` (control.policy.MLPPolicy) once for every environment -> (obs [num_envs, 2 M_o], pre, actions [num_envs, 2M]):
        on obs if given, else on the modes of the current E_mesh (`modes(M_o)`, bit for bit: Re E_1..E_Mo, then Im).  pre is
        u = z + std * eps with noise = eps [num_envs, 2M] (std [2M], None = 1), or u = z; actions a = u, or action_scale tanh(u)
        with squash.  NumPy, or float64 CUDA tensors if an input is one or with on_device.  The state is not touched."""
        mem, spec, keep, obs, noise, std, (o, u, a) = self._policy_call(policy, None, obs, noise, std, on_device)
        mem.enter()
        self._h.policy_eval(spec, mem.addr(obs), mem.addr(noise), mem.addr(std), mem.kind, mem.addr(o), mem.addr(u), mem.addr(a))
        mem.leave(self._h)
        return o, u, a

    def step_policy(self, policy, nsteps: int, noise=None, std=None, history: bool = True, on_device: bool = False):
        """nsteps closed-loop steps under `policy` in ONE call, without returning to the host between steps (pic_step_policy):
        step s evaluates the policy on the field step s-1 left (the current E_mesh for the first), then steps under its actions
        -- bit for bit the host loop `policy_eval` -> `step_actions`.  noise: eps [nsteps, num_envs, 2M] (one torch.randn for the
        whole rollout; the library draws nothing) or None; std [2M] or None.  -> PolicyRollout(obs [nsteps, num_envs, 2 M_o],
        pre, actions [nsteps, num_envs, 2M], KE, PE, PE_reward [nsteps, num_envs] NumPy -- None without history).  NumPy, or
        float64 CUDA tensors if an input is one or with on_device (then asynchronous without history).  Refused while a tape is
        open: tape_step_policy / env.grad.rollout_mlp are the differentiable route (env.grad.rollout_policy for other networks)."""
        from ..control.policy import PolicyRollout
        T = int(nsteps)
        mem, spec, keep, _, noise, std, (o, u, a) = self._policy_call(policy, T, None, noise, std, on_device)
        hist = np.empty((T, 3, self.num_envs)) if history else None
        mem.enter()
        self._h.step_policy(spec, mem.addr(noise), mem.addr(std), mem.kind, T, mem.addr(o), mem.addr(u), mem.addr(a), hist)
        mem.leave(self._h)
        ke, pe, per = (None, None, None) if hist is None else (hist[:, 0], hist[:, 1], hist[:, 2])
        return PolicyRollout(o, u, a, ke, pe, per)

    # -- policy gradients on the device (pic_policy_vjp, pic_tape_step_policy, pic_tape_backward_policy) -----------
    def policy_vjp(self, policy, obs, cot_actions, pre=None, on_device: bool = False):
        """The vector-Jacobian product of `policy_eval` for every environment (pic_policy_vjp): from observations obs
        [num_envs, 2 M_o], the recorded pre (u) [num_envs, 2M] (needed with squash only) and a cotangent cot_actions
        [num_envs, 2M] on the actions -> (g_params [P], or [num_envs, P] with per_env; g_obs [num_envs, 2 M_o]; g_pre
        [num_envs, 2M]).  The gradient with respect to std is sum(g_pre * eps).  NumPy, or float64 CUDA tensors if an input is
        one or with on_device.  The state is not touched."""
        E, nO, nA = self.num_envs, 2 * policy.obs_modes, 2 * self.max_mode
        mem = Mem.of(self, policy.params, obs, pre, cot_actions, force_device=on_device)
        spec, keep = policy.spec(mem, E)
        obs, pre, cot = mem.f64(obs, (E, nO)), mem.f64(pre, (E, nA)), mem.f64(cot_actions, (E, nA))
        gp = mem.empty((E, policy.n_params) if policy.per_env else (policy.n_params,))
        go, gu = mem.empty((E, nO)), mem.empty((E, nA))
        mem.enter()
        self._h.policy_vjp(spec, mem.addr(obs), mem.addr(pre), mem.addr(cot), mem.kind, mem.addr(gp), mem.addr(go), mem.addr(gu))
        mem.leave(self._h)
        del keep
        return gp, go, gu

    def tape_step_policy(self, policy, nsteps: int, noise=None, std=None, history: bool = True, on_device: bool = False):
        """`step_policy` appended to the open tape (pic_tape_step_policy): the same arguments, the same PolicyRollout and the
        same bits, and the steps can be differentiated through the policy by `backward_policy`.  The tape keeps a copy of the
        parameters and every step's observation, pre and action.  All policy calls of one tape must have one shape; they may be
        mixed with step_actions* and step_feedback_gain calls."""
        from ..control.policy import PolicyRollout
        T = int(nsteps)
        mem, spec, keep, _, noise, std, (o, u, a) = self._policy_call(policy, T, None, noise, std, on_device)
        hist = np.empty((T, 3, self.num_envs)) if history else None
        mem.enter()
        self._h.tape_step_policy(spec, mem.addr(noise), mem.addr(std), mem.kind, T, mem.addr(o), mem.addr(u), mem.addr(a), hist)
        mem.leave(self._h)
        self._tape_policy = (2 * policy.obs_modes, policy.n_params, policy.per_env)
        ke, pe, per = (None, None, None) if hist is None else (hist[:, 0], hist[:, 1], hist[:, 2])
        return PolicyRollout(o, u, a, ke, pe, per)

    def backward_policy(self, d_KE=None, d_PE=None, d_PE_reward=None, d_x=None, d_v=None, d_actions=None, d_obs=None,
                        d_KL=None, d_moments=None):
        """`backward` on a tape with steps of `tape_step_policy` (pic_tape_backward_policy): the cotangents of `backward`, plus
        d_actions [T, num_envs, 2M] and d_obs [T, num_envs, 2 M_o], direct cotangents on the policy steps' actions and
        observations (each None = 0).  Returns a dict: "params" ([P], or [num_envs, P] with per_env: the gradient with respect to
        the packed parameters, summed over the tape's policy steps), "pre", "actions" [T, num_envs, 2M] and "obs"
        [T, num_envs, 2 M_o] (u-bar_t, a-bar_t = B^T e-bar_t + d_actions_t and o-bar_t; zero on steps without a policy), "x0",
        "v0" [num_envs, N].  NumPy arrays, or float64 CUDA tensors if any cotangent is one."""
        if getattr(self, "_tape_policy", None) is None:
            raise _abi.PicError("backward_policy: the tape holds no steps of tape_step_policy")
        nO, P, per_env = self._tape_policy
        T, E, N, n = self._h.tape_stats()["steps"], self.num_envs, self.N, 2 * self.max_mode
        mem = Mem.of(self, d_KE, d_PE, d_PE_reward, d_x, d_v, d_actions, d_obs, d_KL, d_moments)
        keep = self._set_kl_cot(d_KL, T, mem), self._set_moments_cot(d_moments, T, mem)
        hist = mem.stack_energies(T, E, d_KE, d_PE, d_PE_reward)
        cx, cv = mem.f64(d_x, (E, N)), mem.f64(d_v, (E, N))
        ca, co = mem.f64(d_actions, (T, E, n)), mem.f64(d_obs, (T, E, nO))
        res = {"params": mem.out((E, P) if per_env else (P,)), "pre": mem.out((T, E, n)), "obs": mem.out((T, E, nO)),
               "actions": mem.out((T, E, n)), "x0": mem.out((E, N)), "v0": mem.out((E, N))}
        addr = mem.addr
        mem.enter()
        self._h.tape_backward_policy(mem.kind, addr(hist), addr(cx), addr(cv), addr(ca), addr(co), addr(res["params"]),
                                     addr(res["pre"]), addr(res["obs"]), addr(res["actions"]), addr(res["x0"]), addr(res["v0"]))
        if mem.on_device:
            self._check_replay("backward_policy", "gradient")
        del keep                                     # (the backward has been waited for)
        return res

    def tape_policy_grad(self, on_device: bool = False):
        """The parameter gradient a finished reverse pass over the tape's policy steps accumulated (pic_tape_policy_grad): after
        `backward`, `backward_policy` or a `TapeWalk` that reached the tape's start."""
        if getattr(self, "_tape_policy", None) is None:
            raise _abi.PicError("tape_policy_grad: the tape holds no steps of tape_step_policy")
        _, P, per_env = self._tape_policy
        mem = Mem.of(self, force_device=on_device)
        out = mem.empty((self.num_envs, P) if per_env else (P,))
        mem.enter()
        self._h.tape_policy_grad(mem.kind, mem.addr(out))
        mem.leave(self._h)
        return out

    # -- forward mode through the policy's steps (pic_policy_jvp, pic_tape_tangent_policy) ---------------------------
    def policy_jvp(self, policy, obs, pre=None, d_params=None, d_obs=None, d_pre=None, on_device: bool = False):
        """The Jacobian-vector product of `policy_eval` for every environment (pic_policy_jvp), dual to `policy_vjp`: from
        observations obs [num_envs, 2 M_o], the recorded pre (u) [num_envs, 2M] (needed with squash only) and the tangents
        d_params [P] (or [num_envs, P] with per_env; `MLPPolicy.pack_tangent` packs layers), d_obs [num_envs, 2 M_o] and d_pre
        [num_envs, 2M], an injection in front of the squash (d_std * eps); each None = 0 -> (d_pre, d_actions) [num_envs, 2M].
        K <= 8 directions at once: every tangent then carries a leading K axis, and so do the results.  NumPy, or float64 CUDA
        tensors if an input is one or with on_device.  The state is not touched."""
        E, nO, nA, P = self.num_envs, 2 * policy.obs_modes, 2 * self.max_mode, policy.n_params
        base = {"d_params": (E, P) if policy.per_env else (P,), "d_obs": (E, nO), "d_pre": (E, nA)}
        given = {k: a for k, a in (("d_params", d_params), ("d_obs", d_obs), ("d_pre", d_pre)) if a is not None}
        K, batched = self._directions("policy_jvp", None, base, given)
        mem = Mem.of(self, policy.params, obs, pre, *given.values(), force_device=on_device)
        spec, keep = policy.spec(mem, E)
        obs, pre = mem.f64(obs, (E, nO)), mem.f64(pre, (E, nA))
        ins = {k: mem.f64(a, (K,) + base[k]) for k, a in given.items()}
        du, da = mem.empty((K, E, nA)), mem.empty((K, E, nA))
        addr = mem.addr
        mem.enter()
        self._h.policy_jvp(spec, addr(obs), addr(pre), K, addr(ins.get("d_params")), addr(ins.get("d_obs")), addr(ins.get("d_pre")),
                           mem.kind, addr(du), addr(da))
        mem.leave(self._h)
        del keep
        return (du, da) if batched else (du[0], da[0])

    def tangent_policy(self, d_params=None, d_std=None, noise=None, d_pre=None, d_actions=None, d_x0=None, d_v0=None,
                       fields: bool = False, on_device: bool = False):
        """Jacobian-vector product of the taped steps through the MLP policy (pic_tape_tangent_policy), dual to
        `backward_policy`: tangents d_params [P] (or [num_envs, P] with per_env) of the parameters of every tape_step_policy call,
        d_std [2M] of std (with noise = eps [T, num_envs, 2M], the rollout's own: d_std * eps is added to d_pre here, the dual of
        g_std = sum g_pre * eps), d_pre and d_actions [T, num_envs, 2M] injections in front of the squash and on the action,
        d_x0, d_v0 [num_envs, N] of the starting particles; each None = 0, and a leading axis of K <= 8 directions as in
        `tangent`.  Returns a dict: "dKE", "dPE", "dPE_reward" [K, T, num_envs], "d_obs" [K, T, num_envs, 2 M_o] (of what step
        t's policy read), "d_pre", "d_actions" [K, T, num_envs, 2M] (d_pre zero on steps without a policy), "d_x", "d_v"
        [K, num_envs, N] (final particles) and, with fields, "d_E_mesh" [K, T, num_envs, N_mesh].  On a mixed tape a
        step_actions* step takes d_actions as its whole tangent and a gain-law step uses its taped gain.  NumPy arrays, or float64
        CUDA tensors if any input is one or with on_device."""
        if getattr(self, "_tape_policy", None) is None:
            raise _abi.PicError("tangent_policy: the tape holds no steps of tape_step_policy")
        nO, P, per_env = self._tape_policy
        T = self._h.tape_stats()["steps"]
        E, N, Ng, n = self.num_envs, self.N, self.N_mesh, 2 * self.max_mode
        if d_std is not None and noise is None:
            raise ValueError("tangent_policy: d_std needs noise, the eps of the rollout")
        base = {"d_params": (E, P) if per_env else (P,), "d_std": (n,), "d_pre": (T, E, n), "d_actions": (T, E, n),
                "d_x0": (E, N), "d_v0": (E, N)}
        given = {k: a for k, a in (("d_params", d_params), ("d_std", d_std), ("d_pre", d_pre), ("d_actions", d_actions),
                                   ("d_x0", d_x0), ("d_v0", d_v0)) if a is not None}
        K, batched = self._directions("tangent_policy", None, base, given)
        mem = Mem.of(self, noise, *given.values(), force_device=on_device)
        ins = {k: mem.f64(a, (K,) + base[k]) for k, a in given.items()}
        if "d_std" in ins:
            inj = ins.pop("d_std").reshape(K, 1, 1, n) * mem.f64(noise, (1, T, E, n))
            ins["d_pre"] = mem.f64(inj + ins["d_pre"] if "d_pre" in ins else inj, (K, T, E, n))
        hist, x, v = mem.out((K, T, 3, E)), mem.out((K, E, N)), mem.out((K, E, N))
        do, du, da = mem.out((K, T, E, nO)), mem.out((K, T, E, n)), mem.out((K, T, E, n))
        em = mem.out((K, T, E, Ng)) if fields else None
        addr = mem.addr
        mem.enter()
        self._walk_serial += 1
        self._h.tape_tangent_policy(K, addr(ins.get("d_params")), addr(ins.get("d_pre")), addr(ins.get("d_actions")),
                                    addr(ins.get("d_x0")), addr(ins.get("d_v0")), mem.kind, addr(hist), addr(do), addr(du), addr(da),
                                    addr(x), addr(v), addr(em))
        if mem.on_device:
            self._check_replay("tangent_policy", "tangent")
        res = {"dKE": hist[:, :, 0], "dPE": hist[:, :, 1], "dPE_reward": hist[:, :, 2], "d_obs": do, "d_pre": du, "d_actions": da,
               "d_x": x, "d_v": v}
        if fields:
            res["d_E_mesh"] = em
        return res if batched else {k: a[0] for k, a in res.items()}

    def modes(self, max_mode: int):
        """Complex [num_envs, max_mode]: rows 1..max_mode of compute_E_k_spectrum for the current E_mesh."""
        return self._h.modes(max_mode)

    def feedback_actions(self, max_mode: int):
        """The linear-feedback / behaviour-cloning action of run_feedback.py:133-135 and ddpg.py:369-371:
        cos coefficients -Re(E_k), sin coefficients +Im(E_k), k = 1..max_mode."""
        ek = self.modes(max_mode)
        return np.concatenate([-ek.real, ek.imag], axis=1)

    # -- stream-ordered operation next to torch (no host synchronisation in the loop) ------------------
    def use_torch_stream(self, stream=None):
        """Run this environment's kernels on torch's current (or the given) stream, so that torch ops
        on that stream and environment steps are ordered by the stream alone."""
        import torch
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        self._h.set_stream(st.cuda_stream)
        self._torch_stream = st

    def use_own_stream(self):
        self._h.own_stream()
        self._torch_stream = None

    def step_actions_torch(self, actions, nsteps: int = 1):
        """actions: float64 CUDA tensor [num_envs, 2*max_mode] on this device; consumed in stream order."""
        if not (actions.is_cuda and actions.dtype.is_floating_point and actions.element_size() == 8
                and actions.is_contiguous() and tuple(actions.shape) == (self.num_envs, 2 * self.max_mode)):
            raise ValueError("actions must be a contiguous float64 CUDA tensor [num_envs, 2*max_mode]")
        shared = self._torch_stream is not None
        if not shared:      # different streams: order them through the host
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._h.step_actions_device(actions.data_ptr(), nsteps)
        if not shared:
            self._h.sync()

    def feedback_actions_torch(self, max_mode: int):
        """`feedback_actions` with everything on the device: returns a float64 CUDA tensor [num_envs, 2*max_mode]."""
        import torch
        dev = f"cuda:{self.device}"
        re = torch.empty((self.num_envs, max_mode), dtype=torch.float64, device=dev)
        im = torch.empty_like(re)
        shared = self._torch_stream is not None
        if not shared:
            torch.cuda.current_stream(self.device).synchronize()
        self._h.modes_device(max_mode, re.data_ptr(), im.data_ptr())
        if not shared:
            self._h.sync()
        return torch.cat([-re, im], dim=1)

    def modes_torch(self, max_mode: int):
        """The modes of the current field as a float64 CUDA tensor [num_envs, 2*max_mode]: Re E_1..E_M, then Im E_1..E_M
        (`modes`' rows, pic_get_modes on the device)."""
        import torch
        re = torch.empty((self.num_envs, max_mode), dtype=torch.float64, device=f"cuda:{self.device}")
        im = torch.empty_like(re)
        shared = self._torch_stream is not None
        if not shared:
            torch.cuda.current_stream(self.device).synchronize()
        self._h.modes_device(max_mode, re.data_ptr(), im.data_ptr())
        if not shared:
            self._h.sync()
        return torch.cat([re, im], dim=1)

    def _ordered_views(self):
        """The zero-copy views, safe to read on torch's current stream: on a shared stream (use_torch_stream) the stream
        orders the read behind the steps; otherwise the handle's own stream is drained first."""
        if not hasattr(self, "_views"):
            self._views = self.torch_views()
        if self._torch_stream is None:
            self._h.sync()
        return self._views

    def energy_views_torch(self):
        """{"KE", "PE", "PE_reward"}: the zero-copy [num_envs] views of the energies the last step left, safe to read on torch's
        current stream (no kernel is launched: the handle's own stream is drained unless it is shared with torch)."""
        v = self._ordered_views()
        return {k: v[k] for k in ("KE", "PE", "PE_reward")}

    def rewards_torch(self):
        """max(1 - PE_reward, 0) per environment as a CUDA tensor (reward.py:72), read from the zero-copy view (after a
        sync of the handle's stream unless it is shared with torch: use_torch_stream)."""
        import torch
        return torch.clamp(1.0 - self._ordered_views()["PE_reward"], min=0.0)

    def trainer_rewards_torch(self, actions=None, alpha: float = 1.0, beta: float = 1.0, r_pe_n: float = 1.0,
                              r_ie_n: Optional[float] = None):
        """Reward.compute_reward (src/control/rl/reward.py:71-76) for every environment, on the device:
        alpha max(1 - PE_r / r_pe_n, 0) + beta max(1 - (sum a^2 L / 4) / r_ie_n, 0), with PE_r the field energy of the
        CURRENT state (read before stepping, it is the pre-step reward the trainers use, ddpg.py:455) and `actions` the
        [num_envs, A] CUDA tensor about to be applied.  r_ie_n defaults to the reference's normaliser, the input energy of
        an all-ones action of the same length (reward.py:26)."""
        import torch
        r = alpha * torch.clamp(1.0 - self._ordered_views()["PE_reward"] / r_pe_n, min=0.0)
        if actions is not None and beta != 0.0:
            a = actions.to(torch.float64)
            ie = (a * a).sum(dim=1) * (self.L * 0.25)
            if r_ie_n is None:
                r_ie_n = a.shape[1] * self.L * 0.25
            r = r + beta * torch.clamp(1.0 - ie / r_ie_n, min=0.0)
        return r

    def phase_density(self, nbins: int, vmin: float = -25.0, vmax: float = 25.0):
        """estimate_f (src/control/objective.py:8-14) for every environment, [num_envs, nbins, nbins]:
        the histogram is counted on the device, the normalisation n0/dx/dv/N applied here."""
        counts = self._h.phase_histogram(nbins, vmin, vmax).astype(np.float64)
        dx, dv = self.L / nbins, (vmax - vmin) / nbins
        counts *= self.n0 / dx / dv / self.N
        return counts

    def kl_divergence(self, feq, vmin: float = -25.0, vmax: float = 25.0):
        """Reward.compute_kl_divergence (reward.py:43-46) of every environment against `feq` [nbins, nbins]: histogram and
        reduction on the device, one value per environment read back (pic_phase_kl)."""
        return self._h.phase_kl(feq, vmin, vmax)

    # -- smoothed phase-space density and KL (pic_phase_kl_smooth*) -----------------------
    def _phase_call(self, feq, *arrays):
        """(the Mem of the call, (nx, nv, feq's address, per-environment flag), feq and the other arrays as float64 in that
        memory): CUDA tensors in, CUDA tensors out, else NumPy.  The call is ordered behind torch on return."""
        mem = Mem.of(self, feq, *arrays)
        f = mem.f64(feq)
        if f.ndim == 3 and f.shape[0] != self.num_envs or f.ndim not in (2, 3):
            raise ValueError(f"feq must be [nx, nv] or [num_envs, nx, nv], not {list(f.shape)}")
        held = [f] + [mem.f64(a) for a in arrays]
        mem.enter()
        return mem, (int(f.shape[-2]), int(f.shape[-1]), mem.addr(f), int(f.ndim == 3)), held

    def phase_density_smooth(self, bins, vmin: float = -25.0, vmax: float = 25.0):
        """The smoothed phase-space density f~ [num_envs, nx, nv] of the current particles: CIC weights on the
        bin centres of [0, L] x [vmin, vmax] (periodic in x, the outer half-bins of v clamped), estimate_f's normalisation and
        mass.  bins: int or (nx, nv), 1..1024 each.  Bitwise reproducible; a target feq for kl_smooth built from an initial state."""
        nx, nv = (int(bins), int(bins)) if np.isscalar(bins) else (int(bins[0]), int(bins[1]))
        f = np.empty((self.num_envs, nx, nv))
        self._h.phase_kl_smooth(nx, nv, vmin, vmax, 0, 0, _abi.PIC_HOST, _abi.PIC_HOST, 0, f.ctypes.data)
        return f

    def kl_smooth(self, feq, vmin: float = -25.0, vmax: float = 25.0):
        """KL~ of every environment's smoothed density against feq [nx, nv] (shared) or [num_envs, nx, nv] ->
        [num_envs]: sum rel_entr(f~, feq + 1e-12) dx dv, estimate_KL_divergence's formula.  NumPy, or a float64 CUDA tensor if
        feq is one."""
        mem, (nx, nv, fa, per), _held = self._phase_call(feq)
        kl = mem.empty((self.num_envs,))
        self._h.phase_kl_smooth(nx, nv, vmin, vmax, fa, per, mem.kind, mem.kind, mem.addr(kl), 0)
        return kl

    def kl_smooth_grad(self, feq, d_kl=None, vmin: float = -25.0, vmax: float = 25.0):
        """Gradient of sum_e d_kl[e] KL~_e (d_kl [num_envs], None = ones) with respect to the current particles -> (g_x, g_v)
        [num_envs, N]: the almost-everywhere derivative of DESIGN.md 7g.  NumPy, or float64 CUDA tensors if feq or d_kl is one."""
        if d_kl is None:
            d_kl = np.ones(self.num_envs)
        mem, (nx, nv, fa, per), (_f, d) = self._phase_call(feq, d_kl)
        if tuple(d.shape) != (self.num_envs,):
            raise ValueError(f"d_kl must be [num_envs], not {list(d.shape)}")
        gx, gv = mem.empty((self.num_envs, self.N)), mem.empty((self.num_envs, self.N))
        self._h.phase_kl_smooth_vjp(nx, nv, vmin, vmax, fa, per, mem.kind, mem.addr(d), mem.kind, mem.addr(gx), mem.addr(gv))
        return gx, gv

    def kl_smooth_jvp(self, feq, vmin: float = -25.0, vmax: float = 25.0, d_x=None, d_v=None):
        """Directional derivatives of KL~ along tangents d_x, d_v [num_envs, N] of the current particles (each None = 0) ->
        [num_envs]: sum_i dKL~/dx_i d_x_i + dKL~/dv_i d_v_i with kl_smooth_grad's derivative (pic_phase_kl_smooth_jvp,
        DESIGN.md 7j).  With a leading axis of K <= 8 directions on the inputs the result is [K, num_envs].  Bitwise
        reproducible.  NumPy, or a float64 CUDA tensor if feq or a tangent is one."""
        E, N = self.num_envs, self.N
        given = [a for a in (d_x, d_v) if a is not None]
        ks = {int(a.shape[0]) for a in given if len(a.shape) == 3}
        if len(ks) > 1:
            raise ValueError(f"kl_smooth_jvp: the inputs disagree on the number of directions: {sorted(ks)}")
        batched = bool(ks)
        K = ks.pop() if ks else 1
        for a in given:
            if tuple(a.shape) != ((K,) if batched else ()) + (E, N):
                raise ValueError(f"kl_smooth_jvp: a tangent must have shape {((K,) if batched else ()) + (E, N)}, not {tuple(a.shape)}")
        mem, (nx, nv, fa, per), (_f, tx, tv) = self._phase_call(feq, d_x, d_v)
        out = mem.empty((K, E))
        self._h.phase_kl_smooth_jvp(nx, nv, vmin, vmax, fa, per, mem.kind, K, mem.addr(tx), mem.addr(tv), mem.kind, mem.addr(out))
        return out if batched else out[0]

    # -- fluid moments on the mesh (pic_moments*) ----------------------------------------
    def moments(self, on_device: bool = False):
        """The fluid moments of the current particles, [num_envs, 3, N_mesh] float64: m0 = s sum W (the density), m1 = s sum W v
        (momentum density), m2 = s sum W v^2 (twice the kinetic-energy density), s = n0 L / (N dx), W the environment's own shape
        function.  Every particle format; bitwise reproducible, whatever blocks_per_env, the schedule, accum_dtype or the
        batch.  NumPy, or a float64 CUDA tensor with on_device."""
        mem = Mem.of(self, force_device=on_device)
        out = mem.empty((self.num_envs, 3, self.N_mesh))
        mem.enter()
        self._h.moments(mem.kind, mem.addr(out))
        mem.leave(self._h)
        return out

    def moments_torch(self):
        """`moments` as a float64 CUDA tensor on torch's current stream: no host synchronisation on a stream shared with torch
        (use_torch_stream), like modes_torch."""
        return self.moments(on_device=True)

    def fluid(self):
        """(n, u, T), each [num_envs, N_mesh]: the density m0, the mean velocity u = m1 / m0 and the temperature
        T = m2 / m0 - u^2 of `moments`; u = T = 0 on a node without particles."""
        m = self.moments()
        n = m[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(n != 0, m[:, 1] / n, 0.0)
            T = np.where(n != 0, m[:, 2] / n - u * u, 0.0)
        return n, u, T

    def moments_vjp(self, g):
        """Gradient of sum g . moments (g [num_envs, 3, N_mesh]) with respect to the current particles -> (g_x, g_v)
        [num_envs, N]: the almost-everywhere derivative of the CIC weights (float64 particles and CIC only).  NumPy, or float64
        CUDA tensors if g is one."""
        mem = Mem.of(self, g)
        c = mem.f64(g)
        if tuple(c.shape) != (self.num_envs, 3, self.N_mesh):
            raise ValueError(f"g must be [num_envs, 3, N_mesh], not {list(c.shape)}")
        gx, gv = mem.empty((self.num_envs, self.N)), mem.empty((self.num_envs, self.N))
        mem.enter()
        self._h.moments_vjp(mem.addr(c), mem.kind, mem.addr(gx), mem.addr(gv))
        return gx, gv

    def moments_jvp(self, d_x=None, d_v=None):
        """Directional derivatives of `moments` along tangents d_x, d_v [num_envs, N] of the current particles (each None = 0) ->
        [num_envs, 3, N_mesh], with moments_vjp's derivative: sum g . moments_jvp(d_x, d_v) = g_x . d_x + g_v . d_v for (g_x, g_v)
        = moments_vjp(g) (pic_moments_jvp).  With a leading axis of K <= 8 directions on the inputs the result is
        [K, num_envs, 3, N_mesh].  Float64 particles and CIC only.  Bitwise reproducible.  NumPy, or a float64 CUDA tensor if a
        tangent is one."""
        E, N = self.num_envs, self.N
        given = [a for a in (d_x, d_v) if a is not None]
        ks = {int(a.shape[0]) for a in given if len(a.shape) == 3}
        if len(ks) > 1:
            raise ValueError(f"moments_jvp: the inputs disagree on the number of directions: {sorted(ks)}")
        batched = bool(ks)
        K = ks.pop() if ks else 1
        for a in given:
            if tuple(a.shape) != ((K,) if batched else ()) + (E, N):
                raise ValueError(f"moments_jvp: a tangent must have shape {((K,) if batched else ()) + (E, N)}, not {tuple(a.shape)}")
        mem = Mem.of(self, d_x, d_v)
        tx, tv = mem.f64(d_x), mem.f64(d_v)
        out = mem.empty((K, E, 3, self.N_mesh))
        mem.enter()
        self._h.moments_jvp(K, mem.addr(tx), mem.addr(tv), mem.kind, mem.addr(out))
        return out if batched else out[0]

    def _set_moments_cot(self, d_moments, T, mem):
        """The moments' cotangents of a backward onto the tape: d_moments [T, num_envs, 3, N_mesh] (row t on the state step t
        left), or None to clear every row, the start's included.  Returns what must stay alive until the backward is done."""
        if d_moments is None:
            if self._tape_moments:
                self._h.tape_moments_cot(0, _abi.PIC_HOST, -1, T + 1)
            return None
        d = mem.f64(d_moments, (T, self.num_envs, 3, self.N_mesh))
        mem.enter()
        self._tape_moments = True
        self._h.tape_moments_cot(0, _abi.PIC_HOST, -1, 1)
        if T > 0:
            self._h.tape_moments_cot(mem.addr(d), mem.kind, 0, T)
        return d

    # -- rollout recorder (include/picstep.h: pic_record_*) ----------------------------------------
    def start_recording(self, stride: int = 1, modes: Optional[int] = None, x_bins: int = 0, v_bins: int = 0, phase_bins=None,
                        vmin: float = -25.0, vmax: float = 25.0, feq=None, capacity: int = 4096, phase_dx: float = 0.0,
                        phase_dv: float = 0.0):
        """Record every `stride`-th step of every stepping call from now on (and `record_now()`), on the device: the energies,
        field_energy = sum(E_mesh^2) dx, spectrum rows 0..modes-1 (default: compute_E_k_spectrum's non-negative k), x / v
        histograms of x_bins / v_bins bins, and from a phase_bins (int or (nx, nv)) histogram on [0, L] x [vmin, vmax] the
        entropy of landau.py:19-25 and, with feq [nx, nv], the KL cost of pic_phase_kl.  A call that would hold more than
        `capacity` records is refused before it steps.  Recording changes no particle, field or energy."""
        self._h.record_start(**recorder_args(self.N_mesh, stride, modes, x_bins, v_bins, phase_bins, vmin, vmax, feq, capacity,
                                             phase_dx, phase_dv))

    def record_now(self):
        """Append a record of the current state (e.g. t = 0 before the first step)."""
        self._h.record_now()

    def recorded(self) -> Record:
        """All records held so far as a Record (they stay held until stop_recording)."""
        c = self._h.record_config
        if c is None:
            raise RuntimeError("recorded(): not recording (start_recording first)")
        return Record._from_read(self._h.record_read(), self.dt, self.L, self.N_mesh, c["vmin"], c["vmax"])

    def stop_recording(self):
        """Stop and free the records (read them with recorded() first)."""
        self._h.record_stop()

    def recording(self, **kwargs):
        """Context manager: start_recording(**kwargs) on entry; on exit the yielded session's `.record` receives recorded()
        and the recorder stops."""
        return recording_session(self, **kwargs)

    def stream_probe(self, repeats=10):
        """GB/s of a read-2-arrays / write-2-arrays copy with the sweeps' grid on this device."""
        return self._h.stream_probe(repeats)

    def bad_count(self):
        return self._h.bad_count()

    def profile(self, enable=True):
        self._h.profile(enable)

    def profile_read(self):
        return self._h.profile_read()

    def torch_views(self):
        """Zero-copy torch tensors over the device state: x, v [num_envs, N] (strided), n, E_mesh,
        phi [num_envs, Ng], KE, PE, PE_reward [num_envs].  Call sync() before reading them on
        another stream.  A write to x or v must be followed by invalidate() or refresh().
        With position_dtype="fixed32" the zero-copy position view is `x_fixed` (int32 bit pattern of the
        uint32 u, x = u L / 2^32) and `x` is a float64 COPY computed from it."""
        import torch

        p = self._h.device_ptrs()
        ts = "<f8" if self.dtype == np.float64 else "<f4"
        isz = self.dtype.itemsize
        dev = f"cuda:{self.device}"
        out = {}
        for k in ("x", "v"):
            t = "<i4" if (k == "x" and self.fixed_positions) else ts
            view = _DeviceView(p[k], (self.num_envs, self.N), t, (p["ld"] * isz, isz))
            out[k] = torch.as_tensor(view, device=dev)
        if self.fixed_positions:
            out["x_fixed"] = out["x"]
            out["x"] = (out["x_fixed"].to(torch.int64) & 0xFFFFFFFF).to(torch.float64) * (self.L / 2.0 ** 32)
        for k in ("n", "E_mesh", "phi"):
            out[k] = torch.as_tensor(_DeviceView(p[k], (self.num_envs, self.N_mesh), "<f8"), device=dev)
        for k in ("KE", "PE", "PE_reward"):
            out[k] = torch.as_tensor(_DeviceView(p[k], (self.num_envs,), "<f8"), device=dev)
        return out

    # -- copies of whole environments (pic_copy_envs) --------------------------------------
    def _copy(self, src, index):
        """copy_envs with the CUDA-tensor rules of step_actions_torch: a tensor map is read in stream order on a shared stream
        (use_torch_stream), otherwise the two streams are ordered through the host."""
        if not hasattr(index, "data_ptr"):
            return self._h.copy_envs(src, index)
        shared = self._torch_stream is not None
        if not shared:
            import torch
            torch.cuda.current_stream(self.device).synchronize()
        self._h.copy_envs(src, index)
        if not shared:
            self._h.sync()               # (the map may be a temporary: it must outlive the kernels that read it)

    def fork(self, index):
        """Environment e becomes a copy of environment index[e], on the device: particles, fields, energies and the cached
        deposit of the next step, so that a copy continues bit for bit like its source.  index[e] == e keeps e; every other
        entry must name a kept environment.  index: a sequence, a NumPy array (checked here: PicError, nothing copied) or an
        int32 CUDA tensor [num_envs] (checked on the device: a wrong entry keeps its environment and counts in
        `copy_rejected`).  Asynchronous."""
        self._copy(self._h, index)

    def copy_from(self, other, index=None):
        """Every environment of this handle becomes a copy of an environment of `other` (a BatchedPIC or a PIC with the same
        N, N_mesh, L, n0, dt, dtypes, interpol, accumulator, integrator and device; num_envs, blocks_per_env and the schedule
        may differ).  index: an int (broadcast that environment to all), an array or int32 CUDA tensor [num_envs] of source
        environments, or None (equal num_envs: environment by environment).  Asynchronous on this handle's stream, ordered
        behind the work queued on `other` and ahead of its later steps."""
        src = other._ensure_handle() if hasattr(other, "_ensure_handle") else other._h
        if index is not None and not hasattr(index, "data_ptr") and np.ndim(index) == 0:
            index = np.full(self.num_envs, int(index), dtype=np.int64)
        self._copy(src, index)

    def copy_rejected(self) -> int:
        """Entries of CUDA-tensor maps that `fork` / `copy_from` refused since this object was created (waits for the stream)."""
        return self._h.copy_envs_rejected()

    def invalidate(self):
        """After a write to x / v through `torch_views()`: drop the cached first deposit of the next step."""
        self._h.invalidate()

    def refresh(self):
        """update_density + update_E_field on the current particles (also valid after a write through the views)."""
        self._h.refresh()

    # -- differentiable rollouts (pic_tape_*) ------------------------------------------
    def start_tape(self, max_steps: int, checkpoint_every: int = 0, budget_bytes: int = 0, kl=None, moments: bool = False):
        """Open a tape: the steps that follow (step, step_history, step_actions[_traj], step_ext_traj, step_observe,
        step_feedback_gain, up to max_steps of them) can be differentiated by `backward`.  checkpoint_every = 0: about
        sqrt(max_steps).  Float64 particles, CIC, Yoshida-4 and the fixed-point accumulator only.  Resets, step_feedback (use
        step_feedback_gain with G0 for a differentiable reference law), staged steps and changes of actuator or integrator are
        refused while it is open.
        kl = dict(feq=..., vmin=-25.0, vmax=25.0) also records the smoothed KL of `kl_smooth` after every step (pic_tape_kl_*,
        DESIGN.md 7h): `tape_kl()` reads the trace and `backward(d_KL=...)` differentiates it.  feq: NumPy or a CUDA tensor,
        [nx, nv] or [num_envs, nx, nv]; the tape keeps a copy.  If the KL's memory does not fit (PicError), the tape stays open
        without one.
        moments=True also records `moments` after every step (pic_tape_moments_start): `tape_moments()` reads the
        trace, `backward(d_moments=...)` and `tangent(moments=True)` differentiate it.  If the trace does not fit (PicError), the
        tape stays open without one."""
        self._h.tape_start(max_steps, checkpoint_every, budget_bytes)
        self._tape_kl = self._tape_moments = self._tape_mom_trace = False
        self._tape_policy = None
        if kl is not None:
            kl = dict(kl)
            feq, vmin, vmax = kl.pop("feq"), float(kl.pop("vmin", -25.0)), float(kl.pop("vmax", 25.0))
            if kl:
                raise ValueError(f"start_tape: unknown keys in kl: {sorted(kl)}")
            mem, (nx, nv, fa, per), _held = self._phase_call(feq)
            self._h.tape_kl_start(nx, nv, vmin, vmax, fa, per, mem.kind)
            self._tape_kl = True
        if moments:
            self._h.tape_moments_start()
            self._tape_mom_trace = True

    def stop_tape(self):
        self._h.tape_stop()
        self._tape_kl = self._tape_moments = self._tape_mom_trace = False
        self._tape_policy = None

    def tape_moments(self, on_device: bool = False):
        """The moments after every step taped so far, [T, num_envs, 3, N_mesh] (a tape opened with moments=True): each row is
        bit for bit what `moments` returns after that step.  NumPy, or a float64 CUDA tensor with on_device."""
        if not self._tape_mom_trace:
            raise _abi.PicError("tape_moments: no tape with a moments trace is open (start_tape(..., moments=True))")
        T = self._h.tape_stats()["steps"]
        mem = Mem.of(self, force_device=on_device)
        out = mem.empty((T, self.num_envs, 3, self.N_mesh))
        if T == 0:
            return out
        mem.enter()
        self._h.tape_moments(mem.kind, mem.addr(out))
        mem.leave(self._h)
        return out

    def tape_kl(self, on_device: bool = False):
        """The smoothed KL after every step taped so far, [T, num_envs] (a tape opened with kl=...): each row is bit for bit
        what kl_smooth returns after that step.  NumPy, or a float64 CUDA tensor with on_device."""
        if not self._tape_kl:
            raise _abi.PicError("tape_kl: no tape with a KL is open (start_tape(..., kl=...))")
        T = self._h.tape_stats()["steps"]
        mem = Mem.of(self, force_device=on_device)
        out = mem.empty((T, self.num_envs))
        if T == 0:
            return out
        mem.enter()
        self._h.tape_kl(mem.kind, mem.addr(out))
        mem.leave(self._h)
        return out

    def _set_kl_cot(self, d_KL, T, mem):
        """The KL cotangents of a backward onto the tape: d_KL [T, num_envs], or None to clear every row.  Returns what must stay
        alive until the backward has been waited for."""
        if not self._tape_kl:
            if d_KL is not None:
                raise ValueError("backward: d_KL needs a tape opened with kl=... (start_tape)")
            return None
        if T == 0:
            return None
        if d_KL is None:
            self._h.tape_kl_cot(0, _abi.PIC_HOST, 0, T)
            return None
        d = mem.f64(d_KL, (T, self.num_envs))
        mem.enter()
        self._h.tape_kl_cot(mem.addr(d), mem.kind, 0, T)
        return d

    def _check_replay(self, who, noun):
        """After a call in device memory: wait for it, and refuse its result if the replay did not reproduce the forward.  (In
        host memory the library itself waits and reports it as the call's error.)"""
        n = self._h.tape_stats()["replay_mismatches"]
        if n:
            raise _abi.PicError(f"{who}: the replay differs from the taped forward in {n} particle values (were the particles "
                                f"written while the tape was open?): the {noun} is not valid")

    def tape_stats(self):
        """steps, checkpoint_every, bytes, replay_mismatches (of the last backward; 0 expected), unit_retries, launches."""
        return self._h.tape_stats()

    def taping(self, max_steps: int, checkpoint_every: int = 0, budget_bytes: int = 0, kl=None, moments: bool = False):
        """Context manager: start_tape(...) on entry, stop_tape() on exit."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            self.start_tape(max_steps, checkpoint_every, budget_bytes, kl=kl, moments=moments)
            try:
                yield self
            finally:
                self.stop_tape()
        return cm()

    def backward(self, d_KE=None, d_PE=None, d_PE_reward=None, d_x=None, d_v=None, d_modes=None, d_KL=None, d_moments=None):
        """Vector-Jacobian product of the taped steps: cotangents d_KE, d_PE, d_PE_reward [T, num_envs] of the energy traces
        (step_history's) and d_x, d_v [num_envs, N] of the final particles (each None = 0).  Returns a dict: "ext" [T, num_envs,
        N_mesh] (gradient with respect to every step's external field), "actions" [T, num_envs, 2*max_mode] (= B^T ext; with an
        actuator), "x0", "v0" [num_envs, N] (initial particles).  NumPy arrays, or float64 CUDA tensors if any cotangent is one
        (then stream-ordered like step_actions_traj_torch).  Raises PicError if the replay of the taped steps does not reproduce
        the forward bit for bit (particles written through the views while taping): such a gradient would be wrong.
        A tape with steps of step_feedback_gain: the gradient includes the path through the law; d_modes
        [T, num_envs, 2*max_mode] are cotangents on their modes (ignored on other steps), and the dict also holds "modes"
        [T, num_envs, 2*max_mode] (the taped m_t, zero on other steps) and "gain": sum over the call's steps of
        actions_t modes_t^T, [num_envs, 2M, 2M] for one gain-law call, a list of them for several.
        A tape opened with kl=...: d_KL [T, num_envs] are cotangents of the KL trace (`tape_kl`); None = 0.  They
        are set on the tape (or all cleared) before the reverse pass, so a backward is a function of its arguments alone.
        d_moments [T, num_envs, 3, N_mesh]: row t is a cotangent on `moments` of the state step t left; None = 0.
        Set or cleared the same way (pic_tape_moments_cot)."""
        T, E, N, n = self._h.tape_stats()["steps"], self.num_envs, self.N, 2 * self.max_mode
        mem = Mem.of(self, d_KE, d_PE, d_PE_reward, d_x, d_v, d_modes, d_KL, d_moments)
        keep_kl = self._set_kl_cot(d_KL, T, mem), self._set_moments_cot(d_moments, T, mem)
        calls = self._h.tape_law_calls()
        if d_modes is not None and not calls:
            raise ValueError("backward: d_modes needs steps of step_feedback_gain on the tape")
        hist = mem.stack_energies(T, E, d_KE, d_PE, d_PE_reward)
        cx, cv, cm = mem.f64(d_x, (E, N)), mem.f64(d_v, (E, N)), mem.f64(d_modes, (T, E, n))
        res = {"ext": mem.out((T, E, self.N_mesh)), "x0": mem.out((E, N)), "v0": mem.out((E, N))}
        if n > 0:
            res["actions"] = mem.out((T, E, n))
        addr = mem.addr
        mem.enter()
        if calls:
            res["modes"] = mem.out((T, E, n))
            self._h._tape_backward_feedback(mem.kind, addr(hist), addr(cx), addr(cv), addr(cm), addr(res["ext"]),
                                            addr(res["actions"]), addr(res["x0"]), addr(res["v0"]), addr(res["modes"]))
        else:
            self._h._tape_backward(mem.kind, addr(hist), addr(cx), addr(cv), addr(res["ext"]), addr(res.get("actions")),
                                   addr(res["x0"]), addr(res["v0"]))
        if mem.on_device:
            self._check_replay("backward", "gradient")
        del keep_kl                                  # (the backward has been waited for)
        if calls:                                    # sum over each gain-law call's steps of actions_t modes_t^T
            g = [sum(res["actions"][s][:, :, None] * res["modes"][s][:, None, :] for s in range(first, first + k))
                 for first, k in calls]
            res["gain"] = g[0] if len(g) == 1 else g
        return res

    def tangent(self, d_ext=None, d_actions=None, d_x0=None, d_v0=None, fields: bool = False, kl: bool = False,
                moments: bool = False):
        """Jacobian-vector product of the taped steps (pic_tape_tangent): tangents d_ext [T, num_envs, N_mesh] of
        every step's external field, or d_actions [T, num_envs, 2*max_mode] of its actions (at most one), and d_x0, d_v0
        [num_envs, N] of the tape's starting particles (each None = 0).  Every input may carry a leading axis of K <= 8
        directions, computed in one call; without one K = 1 and the outputs have no K axis either.  Returns a dict: "KE", "PE",
        "PE_reward" [K, T, num_envs], "x", "v" [K, num_envs, N] (final particles) and, with fields, "E_mesh" [K, T, num_envs,
        N_mesh] (every step's post-step field).  With kl, on a tape opened with kl=..., "KL" [K, T, num_envs] follows: the
        tangents of the trace `tape_kl` returns (pic_tape_tangent_kl; four more kernels per step); every other key
        keeps its bits.  With moments, "moments" [K, T, num_envs, 3, N_mesh] follows: the tangents of `moments` of the state
        every step left (pic_tape_tangent_moments; three more kernels per step; no trace on the tape needed), dual
        to backward(d_moments=...); every other key keeps its bits.  NumPy arrays, or float64 CUDA tensors if any input is one
        (then stream-ordered like backward).  Raises PicError if the replay of the taped steps does not reproduce the forward
        bit for bit."""
        if kl and not self._tape_kl:
            raise _abi.PicError("tangent: kl=True needs a KL on the tape (start_tape(..., kl=...))")
        T = self._h.tape_stats()["steps"]
        E, N, Ng = self.num_envs, self.N, self.N_mesh
        n = 2 * self.max_mode
        base = {"d_ext": (T, E, Ng), "d_actions": (T, E, n), "d_x0": (E, N), "d_v0": (E, N)}
        given = {k: a for k, a in (("d_ext", d_ext), ("d_actions", d_actions), ("d_x0", d_x0), ("d_v0", d_v0)) if a is not None}
        ks = {int(a.shape[0]) for k, a in given.items() if len(a.shape) == len(base[k]) + 1}
        if len(ks) > 1:
            raise ValueError(f"tangent: the inputs disagree on the number of directions: {sorted(ks)}")
        batched = bool(ks)
        K = ks.pop() if ks else 1
        for k, a in given.items():
            want = ((K,) if batched else ()) + base[k]
            if tuple(a.shape) != want:
                raise ValueError(f"tangent: {k} must have shape {want}, not {tuple(a.shape)}")
        mem = Mem.of(self, *given.values())
        ins = {k: mem.f64(a, (K,) + base[k]) for k, a in given.items()}
        hist, x, v = mem.out((K, T, 3, E)), mem.out((K, E, N)), mem.out((K, E, N))
        em = mem.out((K, T, E, Ng)) if fields else None
        dkl = mem.out((K, T, E)) if kl else None
        dmom = mem.out((K, T, E, 3, Ng)) if moments else None
        addr = mem.addr
        mem.enter()
        self._h._tape_tangent(mem.kind, K, addr(ins.get("d_ext")), addr(ins.get("d_actions")), addr(ins.get("d_x0")),
                              addr(ins.get("d_v0")), addr(hist), addr(x), addr(v), addr(em), kl=addr(dkl) if kl else None,
                              moments=addr(dmom) if moments else None)
        if mem.on_device:
            self._check_replay("tangent", "tangent")
        res = {"KE": hist[:, :, 0], "PE": hist[:, :, 1], "PE_reward": hist[:, :, 2], "x": x, "v": v}
        if fields:
            res["E_mesh"] = em
        if kl:
            res["KL"] = dkl
        if moments:
            res["moments"] = dmom
        return res if batched else {k: a[0] for k, a in res.items()}

    def walk(self, obs_modes: Optional[int] = None, on_device: bool = False):
        """The reverse pass of the open tape one step at a time (pic_tape_walk_*): returns a TapeWalk whose
        step(d_energies, d_x, d_v, d_modes) reverses steps T-1, T-2, ... and end(d_x0, d_v0, d_modes0) closes it.  obs_modes
        M_o (default: the actuator's max_mode, else 1) sets the layout of the mode cotangents [num_envs, 2*M_o] (Re E_1..E_Mo,
        then Im, the map of `modes`).  Outputs are float64 CUDA tensors if any cotangent of the call is one or on_device is
        set, NumPy arrays otherwise.  A later step on the environment, another walk or backward abandons this one (PicError)."""
        mo = int(obs_modes) if obs_modes is not None else max(1, self.max_mode)
        return TapeWalk(self, mo, on_device)

    # -- forward mode through closed loops (pic_tape_tangent_walk_*) ------------------------
    def _directions(self, who, K, base, given):
        """The number of directions of a forward-mode call and whether its arrays carry a leading K axis: from K if given (then
        they do), else from the inputs (`given`: name -> array; `base`: name -> shape without K)."""
        ks = {int(a.shape[0]) for k, a in given.items() if len(a.shape) == len(base[k]) + 1}
        if K is not None:
            ks.add(int(K))
        if len(ks) > 1:
            raise ValueError(f"{who}: the inputs disagree on the number of directions: {sorted(ks)}")
        batched = bool(ks)
        K = ks.pop() if ks else 1
        for k, a in given.items():
            want = ((K,) if batched else ()) + base[k]
            if tuple(a.shape) != want:
                raise ValueError(f"{who}: {k} must have shape {want}, not {tuple(a.shape)}")
        return K, batched

    def tangent_walk(self, K=None, obs_modes: Optional[int] = None, d_x0=None, d_v0=None, d_gain=None, on_device: bool = False):
        """The forward-mode pass of the open tape one step at a time, forward in time (pic_tape_tangent_walk_*):
        returns a TangentWalk whose step(d_actions, d_ext) advances steps 0, 1, ... and whose end() returns the final particles'
        tangents.  d_x0, d_v0 [num_envs, N]: tangents of the tape's starting particles; d_gain [num_envs, 2M, 2M]: the tangent
        of the gain of the tape's step_feedback_gain steps (each None = 0).  K <= 8 directions at once: every array then carries
        a leading K axis (K given, or read off the inputs); without one K = 1 and no array has it.  obs_modes M_o (default: the
        actuator's max_mode, else 1; 0 = none) sets the observation's layout [num_envs, 2*M_o] (Re E_1..E_Mo, then Im, the map of
        `modes`); `.d_modes0` holds its tangent at the tape's start.  On a gain-law step the device forms
        d_a = G d_m + d_G m + d_actions itself; between two steps the caller can put any policy's JVP.  The tangents of the
        per-step KL and of the moments are not available step by step.  Outputs are float64 CUDA tensors if any input is one or
        on_device is set, NumPy arrays otherwise.  A later step on the environment, a reverse walk, backward or tangent abandons
        this walk (PicError), and it abandons a reverse walk."""
        mo = int(obs_modes) if obs_modes is not None else max(1, self.max_mode)
        return TangentWalk(self, K, mo, d_x0, d_v0, d_gain, on_device)

    def tangent_feedback(self, d_gain=None, d_x0=None, d_v0=None, d_actions=None, fields: bool = False):
        """Jacobian-vector product of the taped steps through the gain law (pic_tape_tangent_feedback), dual to
        `backward` on a tape with steps of step_feedback_gain: tangents d_gain [num_envs, 2M, 2M] of their gain, d_x0, d_v0
        [num_envs, N] of the starting particles, d_actions [T, num_envs, 2M] added to every step's action (each None = 0; a
        leading axis of K <= 8 directions as in `tangent`).  Returns a dict: "KE", "PE", "PE_reward" [K, T, num_envs], "modes"
        [K, T, num_envs, 2M] (the tangents of the law's m_t, zero on other steps), "actions" [K, T, num_envs, 2M] (the action
        tangents applied), "x", "v" [K, num_envs, N] and, with fields, "E_mesh" [K, T, num_envs, N_mesh].  On a tape without law
        steps it is `tangent` bit for bit."""
        T = self._h.tape_stats()["steps"]
        E, N, Ng, n = self.num_envs, self.N, self.N_mesh, 2 * self.max_mode
        base = {"d_gain": (E, n, n), "d_x0": (E, N), "d_v0": (E, N), "d_actions": (T, E, n)}
        given = {k: a for k, a in (("d_gain", d_gain), ("d_x0", d_x0), ("d_v0", d_v0), ("d_actions", d_actions)) if a is not None}
        K, batched = self._directions("tangent_feedback", None, base, given)
        mem = Mem.of(self, *given.values())
        ins = {k: mem.f64(a, (K,) + base[k]) for k, a in given.items()}
        hist, x, v = mem.out((K, T, 3, E)), mem.out((K, E, N)), mem.out((K, E, N))
        dm = mem.out((K, T, E, n)) if n else None
        da = mem.out((K, T, E, n)) if n else None
        em = mem.out((K, T, E, Ng)) if fields else None
        addr = mem.addr
        mem.enter()
        self._walk_serial += 1
        self._h.tape_tangent_feedback(K, addr(ins.get("d_gain")), addr(ins.get("d_x0")), addr(ins.get("d_v0")),
                                      addr(ins.get("d_actions")), mem.kind, addr(hist), addr(dm), addr(da), addr(x), addr(v), addr(em))
        if mem.on_device:
            self._check_replay("tangent_feedback", "tangent")
        res = {"KE": hist[:, :, 0], "PE": hist[:, :, 1], "PE_reward": hist[:, :, 2], "x": x, "v": v}
        if n:
            res["modes"], res["actions"] = dm, da
        if fields:
            res["E_mesh"] = em
        return res if batched else {k: a[0] for k, a in res.items()}

    def close(self):
        self._h.close()


class TangentWalk:
    """A forward-mode walk over an open tape (BatchedPIC.tangent_walk)."""

    def __init__(self, env, K, obs_modes, d_x0=None, d_v0=None, d_gain=None, on_device=False):
        E, N, n = env.num_envs, env.N, 2 * env.max_mode
        base = {"d_x0": (E, N), "d_v0": (E, N), "d_gain": (E, n, n)}
        given = {k: a for k, a in (("d_x0", d_x0), ("d_v0", d_v0), ("d_gain", d_gain)) if a is not None}
        self.K, self.batched = env._directions("tangent_walk", K, base, given)
        self.env, self.obs_modes, self.on_device = env, int(obs_modes), bool(on_device)
        mem = Mem.of(env, *given.values(), force_device=self.on_device)
        ins = {k: mem.f64(a, (self.K,) + base[k]) for k, a in given.items()}
        m0 = mem.out((self.K, E, 2 * self.obs_modes)) if self.obs_modes > 0 else None
        mem.enter()
        env._h.tape_tangent_walk_begin(self.K, self.obs_modes, mem.addr(ins.get("d_x0")), mem.addr(ins.get("d_v0")),
                                       mem.addr(ins.get("d_gain")), mem.kind, mem.addr(m0))
        mem.leave(env._h)                            # (the inputs above are alive until here)
        env._walk_serial += 1                        # (a reverse walk in progress is abandoned)
        self._serial = env._walk_serial
        self.d_modes0 = m0 if self.batched or m0 is None else m0[0]

    def _live(self, who):
        if self.env._walk_serial != self._serial:
            raise _abi.PicError(f"tangent_walk.{who}: another walk, backward or tangent has replaced this one")

    def step(self, d_actions=None, d_ext=None, state: bool = False, fields: bool = False):
        """Advance the next step t under this step's injection d_actions [num_envs, 2*max_mode] or d_ext [num_envs, N_mesh] (at
        most one; on a gain-law step d_actions is added to the law's own action tangent and d_ext is refused).  Returns a dict:
        "t", "KE", "PE", "PE_reward" [num_envs], "modes" [num_envs, 2*M_o] (the tangent of the observation of the field the step
        left; with M_o > 0), "actions" [num_envs, 2*max_mode] (the action tangent applied; with an actuator) and, with state,
        "x", "v" [num_envs, N], with fields, "E_mesh" [num_envs, N_mesh]; each with the walk's leading K axis, if it has one."""
        self._live("step")
        env, K, E = self.env, self.K, self.env.num_envs
        n = 2 * env.max_mode
        base = {"d_actions": (E, n), "d_ext": (E, env.N_mesh)}
        given = {k: a for k, a in (("d_actions", d_actions), ("d_ext", d_ext)) if a is not None}
        for k, a in given.items():
            want = ((K,) if self.batched else ()) + base[k]
            if tuple(a.shape) != want:
                raise ValueError(f"tangent_walk.step: {k} must have shape {want}, not {tuple(a.shape)}")
        mem = Mem.of(env, *given.values(), force_device=self.on_device)
        ins = {k: mem.f64(a, (K,) + base[k]) for k, a in given.items()}
        en = mem.out((K, 3, E))
        mo = mem.out((K, E, 2 * self.obs_modes)) if self.obs_modes > 0 else None
        ao = mem.out((K, E, n)) if n else None
        x, v = (mem.out((K, E, env.N)), mem.out((K, E, env.N))) if state else (None, None)
        em = mem.out((K, E, env.N_mesh)) if fields else None
        addr = mem.addr
        mem.enter()
        t = env._h.tape_tangent_walk_step(addr(ins.get("d_ext")), addr(ins.get("d_actions")), mem.kind, addr(en), addr(mo), addr(ao),
                                          addr(x), addr(v), addr(em))
        mem.leave(env._h)                            # (the injections above are alive until here)
        res = {"KE": en[:, 0], "PE": en[:, 1], "PE_reward": en[:, 2]}
        for k, a in (("modes", mo), ("actions", ao), ("x", x), ("v", v), ("E_mesh", em)):
            if a is not None:
                res[k] = a
        if not self.batched:
            res = {k: a[0] for k, a in res.items()}
        res["t"] = t
        return res

    def end(self):
        """After all steps: the tangents of the final particles, (d_x, d_v) [num_envs, N] (with the walk's K axis, if any).
        Raises PicError if a replay of the walk differed from the taped forward."""
        self._live("end")
        env = self.env
        mem = Mem.of(env, force_device=self.on_device)
        x, v = mem.out((self.K, env.num_envs, env.N)), mem.out((self.K, env.num_envs, env.N))
        mem.enter()
        env._h.tape_tangent_walk_end(mem.kind, mem.addr(x), mem.addr(v))
        if mem.on_device:
            env._check_replay("tangent_walk.end", "tangent")
        return (x, v) if self.batched else (x[0], v[0])


class TapeWalk:
    """A reverse walk over an open tape (BatchedPIC.walk)."""

    def __init__(self, env, obs_modes, on_device=False):
        self.env, self.obs_modes, self.on_device = env, int(obs_modes), bool(on_device)
        env._h.tape_walk_begin(self.obs_modes)
        env._walk_serial += 1
        self._serial = env._walk_serial
        # a tape with a KL: the step each call reverses, for its row of KL cotangents
        self._kl_next = env._h.tape_stats()["steps"] - 1 if env._tape_kl else None
        self._steps, self._done = None, 0                      # the tape's steps (read when first needed), the steps reversed so far
        if env._tape_moments:                                  # rows an earlier backward or walk left: this walk sets its own
            env._h.tape_moments_cot(0, _abi.PIC_HOST, -1, self._tape_steps() + 1)

    def _tape_steps(self):
        if self._steps is None:
            self._steps = self.env._h.tape_stats()["steps"]
        return self._steps

    def _live(self, who):
        if self.env._walk_serial != self._serial:
            raise _abi.PicError(f"walk.{who}: another walk or backward has replaced this one")

    def step(self, d_energies=None, d_x=None, d_v=None, d_modes=None, d_kl=None, d_moments=None):
        """Reverse the next step t: d_energies [3, num_envs] (its KE, PE, PE_reward), d_x, d_v [num_envs, N] on the state it
        left, d_modes [num_envs, 2*M_o] on the modes of the field it left, d_kl [num_envs] on its smoothed KL (a tape opened
        with kl=...; None = 0), d_moments [num_envs, 3, N_mesh] on the moments of the state it left (None = 0).  Returns
        (t, g_ext [num_envs, N_mesh], g_actions [num_envs, 2*max_mode] or None without an actuator)."""
        self._live("step")
        env, E = self.env, self.env.num_envs
        if d_kl is not None and self._kl_next is None:
            raise ValueError("walk.step: d_kl needs a tape opened with kl=... (start_tape)")
        mem = Mem.of(env, d_energies, d_x, d_v, d_modes, d_kl, d_moments, force_device=self.on_device)
        ce, cx, cv = mem.f64(d_energies, (3, E)), mem.f64(d_x, (E, env.N)), mem.f64(d_v, (E, env.N))
        cm, ck = mem.f64(d_modes, (E, 2 * self.obs_modes)), mem.f64(d_kl, (E,))
        cf = mem.f64(d_moments, (E, 3, env.N_mesh))
        g_ext = mem.out((E, env.N_mesh))
        g_act = mem.out((E, 2 * env.max_mode)) if env.max_mode > 0 else None
        addr = mem.addr
        mem.enter()
        if self._kl_next is not None and self._kl_next >= 0:
            env._h.tape_kl_cot(addr(ck), _abi.PIC_HOST if ck is None else mem.kind, self._kl_next, 1)
            self._kl_next -= 1
        if cf is not None:
            env._tape_moments = True
            env._h.tape_moments_cot(addr(cf), mem.kind, self._tape_steps() - 1 - self._done, 1)
        self._done += 1
        t = env._h.tape_walk_step(addr(ce), addr(cx), addr(cv), addr(cm), mem.kind, addr(g_ext), addr(g_act))
        mem.leave(env._h)                            # (the cotangents above are alive until here)
        return t, g_ext, g_act

    def end(self, d_x0=None, d_v0=None, d_modes0=None, d_moments0=None):
        """After all steps: cotangents on the tape's starting state, on the modes of the field there and on its moments
        (d_moments0 [num_envs, 3, N_mesh]); returns (g_x0, g_v0) [num_envs, N].  Raises PicError if a replay of the walk differed
        from the taped forward."""
        self._live("end")
        env, E = self.env, self.env.num_envs
        mem = Mem.of(env, d_x0, d_v0, d_modes0, d_moments0, force_device=self.on_device)
        cx, cv, cm = mem.f64(d_x0, (E, env.N)), mem.f64(d_v0, (E, env.N)), mem.f64(d_modes0, (E, 2 * self.obs_modes))
        cf = mem.f64(d_moments0, (E, 3, env.N_mesh))
        g_x0, g_v0 = mem.out((E, env.N)), mem.out((E, env.N))
        addr = mem.addr
        mem.enter()
        if cf is not None:
            env._tape_moments = True
            env._h.tape_moments_cot(addr(cf), mem.kind, -1, 1)
        env._h.tape_walk_end(addr(cx), addr(cv), addr(cm), mem.kind, addr(g_x0), addr(g_v0))
        if mem.on_device:
            env._check_replay("walk.end", "gradient")
        return g_x0, g_v0
