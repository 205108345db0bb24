"""The differentiation layer of `BatchedPIC`: tapes and their reverse and forward passes, the MLP policy's
calls with their VJP and JVP, the smoothed phase-space KL and the fluid moments with their derivatives, and the two stepwise
walks.  `TapePIC` is the base class `BatchedPIC` (env/batched.py) inherits these methods from; every array goes through `Mem`
and every K axis through `directions` (env/_arrays.py).
"""
from typing import Optional

import numpy as np

from .. import _abi
from ._arrays import Mem, directions


class TapePIC:
    def _no_tape(self):
        self._tape_kl = False                # (the open tape records the smoothed KL)
        self._tape_moments = False           # (the open tape has held cotangents on the moments)
        self._tape_mom_trace = False         # (the open tape records the moments of every step)
        self._tape_policy = None             # (obs width, P, per_env) of the open tape's policy steps

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
        self._no_tape()
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
        self._no_tape()

    def _tape_trace(self, recorded, refusal, row, read, on_device):
        """A trace the open tape recorded, [T] + row, read by the Handle method `read`; PicError(refusal) unless `recorded`."""
        if not recorded:
            raise _abi.PicError(refusal)
        T = self._h.tape_stats()["steps"]
        mem = Mem.of(self, force_device=on_device)
        out = mem.empty((T,) + row)
        if T == 0:
            return out
        mem.enter()
        read(mem.kind, mem.addr(out))
        mem.leave(self._h)
        return out

    def tape_moments(self, on_device: bool = False):
        """The moments after every step taped so far, [T, num_envs, 3, N_mesh] (a tape opened with moments=True): each row is
        bit for bit what `moments` returns after that step.  NumPy, or a float64 CUDA tensor with on_device."""
        return self._tape_trace(self._tape_mom_trace, "tape_moments: no tape with a moments trace is open (start_tape(..., "
                                "moments=True))", (self.num_envs, 3, self.N_mesh), self._h.tape_moments, on_device)

    def tape_kl(self, on_device: bool = False):
        """The smoothed KL after every step taped so far, [T, num_envs] (a tape opened with kl=...): each row is bit for bit
        what kl_smooth returns after that step.  NumPy, or a float64 CUDA tensor with on_device."""
        return self._tape_trace(self._tape_kl, "tape_kl: no tape with a KL is open (start_tape(..., kl=...))", (self.num_envs,),
                                self._h.tape_kl, on_device)

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

    def _tape_pass(self, who, noun, mem, base, given, outs, call, K=None, batched=True, bump=False,
                   energies=("KE", "PE", "PE_reward")):
        """One whole pass over the tape, from its description to the result dict.  given: name -> input (None = absent) with
        base: name -> its shape; outs: key -> shape (None = not asked for); call(i, o) makes the Handle call, i[name] / o[key]
        being the addresses in `mem` (0 for an absent one).  K (forward mode): every shape gets a leading K axis, "hist"
        [K, T, 3, num_envs] comes back under the three keys of `energies`, and without `batched` the results lose the axis again.
        bump: the pass abandons the walk in progress.  In device memory the pass is waited for and its replay checked (`noun`
        names the result in the refusal)."""
        lead = () if K is None else (K,)
        ins = {k: mem.f64(a, lead + base[k]) for k, a in given.items()}
        res = {k: mem.out(lead + shape) for k, shape in outs.items() if shape is not None}
        mem.enter()
        if bump:
            self._walk_serial += 1
        call({k: mem.addr(ins.get(k)) for k in base}, {k: mem.addr(res.get(k)) for k in outs})
        if mem.on_device:
            self._check_replay(who, noun)
        if K is None:
            return res
        hist = res.pop("hist")
        res = {**{k: hist[:, :, j] for j, k in enumerate(energies)}, **res}
        return res if batched else {k: a[0] for k, a in res.items()}

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
        base = {"hist": (T, 3, E), "d_x": (E, N), "d_v": (E, N), "d_modes": (T, E, n)}
        given = {"hist": mem.stack_energies(T, E, d_KE, d_PE, d_PE_reward), "d_x": d_x, "d_v": d_v, "d_modes": d_modes}
        outs = {"ext": (T, E, self.N_mesh), "x0": (E, N), "v0": (E, N), "actions": (T, E, n) if n > 0 else None,
                "modes": (T, E, n) if calls else None}

        def call(i, o):
            if calls:
                self._h._tape_backward_feedback(mem.kind, i["hist"], i["d_x"], i["d_v"], i["d_modes"], o["ext"], o["actions"],
                                                o["x0"], o["v0"], o["modes"])
            else:
                self._h._tape_backward(mem.kind, i["hist"], i["d_x"], i["d_v"], o["ext"], o["actions"], o["x0"], o["v0"])
        res = self._tape_pass("backward", "gradient", mem, base, given, outs, call)
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
        given = {"d_ext": d_ext, "d_actions": d_actions, "d_x0": d_x0, "d_v0": d_v0}
        K, batched = directions("tangent", base, given)
        mem = Mem.of(self, *given.values())
        outs = {"hist": (T, 3, E), "x": (E, N), "v": (E, N), "E_mesh": (T, E, Ng) if fields else None,
                "KL": (T, E) if kl else None, "moments": (T, E, 3, Ng) if moments else None}

        def call(i, o):
            self._h._tape_tangent(mem.kind, K, i["d_ext"], i["d_actions"], i["d_x0"], i["d_v0"], o["hist"], o["x"], o["v"],
                                  o["E_mesh"], kl=o["KL"] if kl else None, moments=o["moments"] if moments else None)
        return self._tape_pass("tangent", "tangent", mem, base, given, outs, call, K, batched)

    def walk(self, obs_modes: Optional[int] = None, on_device: bool = False):
        """The reverse pass of the open tape one step at a time (pic_tape_walk_*): returns a TapeWalk whose
        step(d_energies, d_x, d_v, d_modes) reverses steps T-1, T-2, ... and end(d_x0, d_v0, d_modes0) closes it.  obs_modes
        M_o (default: the actuator's max_mode, else 1) sets the layout of the mode cotangents [num_envs, 2*M_o] (Re E_1..E_Mo,
        then Im, the map of `modes`).  Outputs are float64 CUDA tensors if any cotangent of the call is one or on_device is
        set, NumPy arrays otherwise.  A later step on the environment, another walk or backward abandons this one (PicError)."""
        mo = int(obs_modes) if obs_modes is not None else max(1, self.max_mode)
        return TapeWalk(self, mo, on_device)

    # -- forward mode through closed loops (pic_tape_tangent_walk_*) ------------------------
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
        given = {"d_gain": d_gain, "d_x0": d_x0, "d_v0": d_v0, "d_actions": d_actions}
        K, batched = directions("tangent_feedback", base, given)
        mem = Mem.of(self, *given.values())
        outs = {"hist": (T, 3, E), "x": (E, N), "v": (E, N), "modes": (T, E, n) if n else None,
                "actions": (T, E, n) if n else None, "E_mesh": (T, E, Ng) if fields else None}

        def call(i, o):
            self._h.tape_tangent_feedback(K, i["d_gain"], i["d_x0"], i["d_v0"], i["d_actions"], mem.kind, o["hist"], o["modes"],
                                          o["actions"], o["x"], o["v"], o["E_mesh"])
        return self._tape_pass("tangent_feedback", "tangent", mem, base, given, outs, call, K, batched, bump=True)

    # -- closed loops under an MLP policy on the device (pic_policy_eval, pic_step_policy) ------------------
    def _head_call(self, mem, T, row, noise, std, history, call):
        """What a call of either controller shares, the MLP policy's and the particle actor's: noise and std as float64 arrays
        of `mem`, fresh outputs -- the controller's own rows [num_envs, row], pre and actions [num_envs, 2M], behind a leading T
        axis for a rollout of T steps (T None: one evaluation) -- and with `history` the energies' record.  `call` is the Handle
        method with the arguments in front of noise bound: it gets the tail every such entry has, (noise, std, mem_kind, own,
        pre, actions) for an evaluation and (noise, std, mem_kind, T, own, pre, actions, hist) for a rollout, between mem.enter()
        and mem.leave().  -> (own, pre, actions, KE, PE, PE_reward), the last three [T, num_envs] NumPy, or None without history."""
        E, nA = self.num_envs, 2 * self.max_mode
        lead = () if T is None else (T,)
        noise, std = mem.f64(noise, lead + (E, nA)), mem.f64(std, (nA,))
        outs = mem.empty(lead + (E, row)), mem.empty(lead + (E, nA)), mem.empty(lead + (E, nA))
        hist = np.empty((T, 3, E)) if history else None
        mem.enter()
        call(mem.addr(noise), mem.addr(std), mem.kind, *lead, *(mem.addr(a) for a in outs), *(() if T is None else (hist,)))
        mem.leave(self._h)
        return outs + ((None, None, None) if hist is None else (hist[:, 0], hist[:, 1], hist[:, 2]))

    def _policy_call(self, call, policy, T, obs, noise, std, history, on_device):
        """`_head_call` for the policy: `call` is Handle.policy_eval (T None; it takes the observation) or one of the rollouts."""
        E, nO = self.num_envs, 2 * policy.obs_modes
        mem = Mem.of(self, policy.params, obs, noise, std, force_device=on_device)
        spec, keep = policy.spec(mem, E)
        obs = mem.f64(obs, (E, nO))
        front = (spec, mem.addr(obs)) if T is None else (spec,)
        return self._head_call(mem, T, nO, noise, std, history, lambda *tail: call(*front, *tail))

    def policy_eval(self, policy, obs=None, noise=None, std=None, on_device: bool = False):
        """`policy` (control.policy.MLPPolicy) once for every environment -> (obs [num_envs, 2 M_o], pre, actions [num_envs, 2M]):
        on obs if given, else on the modes of the current E_mesh (`modes(M_o)`, bit for bit: Re E_1..E_Mo, then Im).  pre is
        u = z + std * eps with noise = eps [num_envs, 2M] (std [2M], None = 1), or u = z; actions a = u, or action_scale tanh(u)
        with squash.  NumPy, or float64 CUDA tensors if an input is one or with on_device.  The state is not touched."""
        return self._policy_call(self._h.policy_eval, policy, None, obs, noise, std, False, on_device)[:3]

    def step_policy(self, policy, nsteps: int, noise=None, std=None, history: bool = True, on_device: bool = False):
        """nsteps closed-loop steps under `policy` in ONE call, without returning to the host between steps (pic_step_policy):
        step s evaluates the policy on the field step s-1 left (the current E_mesh for the first), then steps under its actions
        -- bit for bit the host loop `policy_eval` -> `step_actions`.  noise: eps [nsteps, num_envs, 2M] (one torch.randn for the
        whole rollout; the library draws nothing) or None; std [2M] or None.  -> PolicyRollout(obs [nsteps, num_envs, 2 M_o],
        pre, actions [nsteps, num_envs, 2M], KE, PE, PE_reward [nsteps, num_envs] NumPy -- None without history).  NumPy, or
        float64 CUDA tensors if an input is one or with on_device (then asynchronous without history).  Refused while a tape is
        open: tape_step_policy / env.grad.rollout_mlp are the differentiable route (env.grad.rollout_policy for other networks)."""
        return self._rollout_policy(self._h.step_policy, policy, nsteps, noise, std, history, on_device)

    def _rollout_policy(self, step, policy, nsteps, noise, std, history, on_device):
        """step_policy and tape_step_policy: `step` is the Handle method of the one or the other."""
        from ..control.policy import PolicyRollout
        return PolicyRollout(*self._policy_call(step, policy, int(nsteps), None, noise, std, history, on_device))

    # -- closed loops under the DeepSets particle actor (pic_actor_eval, pic_step_actor) -------------------------
    def _actor_call(self, who, actor, T, features, x, v, noise, std, history, on_device):
        """`_head_call` for the actor: `who` names the Handle method, actor_eval (T None; it takes features, x and v) or
        step_actor.  Every shape is checked here, before the handle or the device is touched."""
        E, N, H, nA = self.num_envs, self.N, actor.hidden, 2 * self.max_mode
        lead = () if T is None else (T,)
        if T is not None and T < 0:
            raise ValueError(f"{who}: nsteps must be >= 0, not {T}")
        if self.max_mode and actor.widths[-1] != nA:          # (without an actuator the library refuses: PIC_ESTATE)
            raise ValueError(f"{who}: the actor's last width must be 2 max_mode of the actuator = {nA}, not {actor.widths[-1]}")
        if actor.per_env and actor.W.shape[0] != E:
            raise ValueError(f"{who}: a per-environment actor needs parameters for {E} environments, not {actor.W.shape[0]}")
        if features is not None and (x is not None or v is not None):
            raise ValueError(f"{who}: features must not be given together with x or v")
        if (x is None) != (v is None):
            raise ValueError(f"{who}: x and v must both be given or both be None")
        for name, a, want in (("features", features, (E, H)), ("x", x, (E, N)), ("v", v, (E, N)), ("noise", noise, lead + (E, nA)),
                              ("std", std, (nA,))):
            if a is not None and tuple(np.shape(a)) != want:
                raise ValueError(f"{who}: {name} must have shape {list(want)}, not {list(np.shape(a))}")
        mem = Mem.of(self, actor.params, features, x, v, noise, std, force_device=on_device)
        spec, keep = actor.spec(mem, E)
        ins = [mem.f64(a) for a in (features, x, v)]
        front = (spec, *(mem.addr(a) for a in ins)) if T is None else (spec,)
        return self._head_call(mem, T, H, noise, std, history, lambda *tail: getattr(self._h, who)(*front, *tail))

    def actor_eval(self, actor, features=None, x=None, v=None, noise=None, std=None, on_device: bool = False):
        """`actor` (control.actor.ParticleActor) once for every environment -> (features [num_envs, H], pre, actions
        [num_envs, 2M]): on features [num_envs, H] if given (the head alone), else on the particles x, v [num_envs, N], else on
        the stored particles of a float64 environment -- the features are then `pool(...)`'s for the actor's pool part, bit for
        bit.  pre is u = z + std * eps with noise = eps [num_envs, 2M] (std [2M], None = 1), or u = z; actions a = u, or
        action_shift + action_scale tanh(u) with squash.  NumPy, or float64 CUDA tensors if an input is one or with on_device.
        The state is not touched."""
        return self._actor_call("actor_eval", actor, None, features, x, v, noise, std, False, on_device)[:3]

    def step_actor(self, actor, nsteps: int, noise=None, std=None, history: bool = True, on_device: bool = False):
        """nsteps closed-loop steps under `actor` in ONE call, without returning to the host between steps (pic_step_actor): step
        s evaluates the actor on the particles step s-1 left (the stored ones for the first), then steps under its actions --
        bit for bit the host loop `pool` -> `actor_eval(features=...)` -> `step_actions`.  noise: eps [nsteps, num_envs, 2M] (the
        library draws nothing) or None; std [2M] or None.  -> ActorRollout(features [nsteps, num_envs, H], pre, actions
        [nsteps, num_envs, 2M], KE, PE, PE_reward [nsteps, num_envs] NumPy -- None without history).  NumPy, or float64 CUDA
        tensors if an input is one or with on_device (then asynchronous without history).  Float64 environments only.  Refused
        while a tape is open: `actor.to_torch(env)` under env.grad.rollout_policy(observe="state") is the differentiable route."""
        from ..control.actor import ActorRollout
        return ActorRollout(*self._actor_call("step_actor", actor, int(nsteps), None, None, None, noise, std, history, on_device))

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
        out = self._rollout_policy(self._h.tape_step_policy, policy, nsteps, noise, std, history, on_device)
        self._tape_policy = (2 * policy.obs_modes, policy.n_params, policy.per_env)
        return out

    def _policy_steps(self, who):
        """(obs width, P, per_env) of the open tape's policy steps; PicError if it has none."""
        if self._tape_policy is None:
            raise _abi.PicError(f"{who}: the tape holds no steps of tape_step_policy")
        return self._tape_policy

    def backward_policy(self, d_KE=None, d_PE=None, d_PE_reward=None, d_x=None, d_v=None, d_actions=None, d_obs=None,
                        d_KL=None, d_moments=None):
        """`backward` on a tape with steps of `tape_step_policy` (pic_tape_backward_policy): the cotangents of `backward`, plus
        d_actions [T, num_envs, 2M] and d_obs [T, num_envs, 2 M_o], direct cotangents on the policy steps' actions and
        observations (each None = 0).  Returns a dict: "params" ([P], or [num_envs, P] with per_env: the gradient with respect to
        the packed parameters, summed over the tape's policy steps), "pre", "actions" [T, num_envs, 2M] and "obs"
        [T, num_envs, 2 M_o] (u-bar_t, a-bar_t = B^T e-bar_t + d_actions_t and o-bar_t; zero on steps without a policy), "x0",
        "v0" [num_envs, N].  NumPy arrays, or float64 CUDA tensors if any cotangent is one."""
        nO, P, per_env = self._policy_steps("backward_policy")
        T, E, N, n = self._h.tape_stats()["steps"], self.num_envs, self.N, 2 * self.max_mode
        mem = Mem.of(self, d_KE, d_PE, d_PE_reward, d_x, d_v, d_actions, d_obs, d_KL, d_moments)
        keep = self._set_kl_cot(d_KL, T, mem), self._set_moments_cot(d_moments, T, mem)
        base = {"hist": (T, 3, E), "d_x": (E, N), "d_v": (E, N), "d_actions": (T, E, n), "d_obs": (T, E, nO)}
        given = {"hist": mem.stack_energies(T, E, d_KE, d_PE, d_PE_reward), "d_x": d_x, "d_v": d_v, "d_actions": d_actions,
                 "d_obs": d_obs}
        outs = {"params": (E, P) if per_env else (P,), "pre": (T, E, n), "obs": (T, E, nO), "actions": (T, E, n), "x0": (E, N),
                "v0": (E, N)}

        def call(i, o):
            self._h.tape_backward_policy(mem.kind, i["hist"], i["d_x"], i["d_v"], i["d_actions"], i["d_obs"], o["params"], o["pre"],
                                         o["obs"], o["actions"], o["x0"], o["v0"])
        res = self._tape_pass("backward_policy", "gradient", mem, base, given, outs, call)
        del keep                                     # (the backward has been waited for)
        return res

    def tape_policy_grad(self, on_device: bool = False):
        """The parameter gradient a finished reverse pass over the tape's policy steps accumulated (pic_tape_policy_grad): after
        `backward`, `backward_policy` or a `TapeWalk` that reached the tape's start."""
        _, P, per_env = self._policy_steps("tape_policy_grad")
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
        given = {"d_params": d_params, "d_obs": d_obs, "d_pre": d_pre}
        K, batched = directions("policy_jvp", base, given)
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
        nO, P, per_env = self._policy_steps("tangent_policy")
        T = self._h.tape_stats()["steps"]
        E, N, Ng, n = self.num_envs, self.N, self.N_mesh, 2 * self.max_mode
        if d_std is not None and noise is None:
            raise ValueError("tangent_policy: d_std needs noise, the eps of the rollout")
        base = {"d_params": (E, P) if per_env else (P,), "d_std": (n,), "d_pre": (T, E, n), "d_actions": (T, E, n),
                "d_x0": (E, N), "d_v0": (E, N)}
        given = {"d_params": d_params, "d_std": d_std, "d_pre": d_pre, "d_actions": d_actions, "d_x0": d_x0, "d_v0": d_v0}
        K, batched = directions("tangent_policy", base, given)
        mem = Mem.of(self, noise, *given.values(), force_device=on_device)
        if d_std is not None:                        # d_std * eps joins d_pre, in front of the squash
            inj = mem.f64(given.pop("d_std"), (K, 1, 1, n)) * mem.f64(noise, (1, T, E, n))
            given["d_pre"] = inj + mem.f64(d_pre, (K, T, E, n)) if d_pre is not None else inj
        outs = {"hist": (T, 3, E), "d_obs": (T, E, nO), "d_pre": (T, E, n), "d_actions": (T, E, n), "d_x": (E, N), "d_v": (E, N),
                "d_E_mesh": (T, E, Ng) if fields else None}

        def call(i, o):
            self._h.tape_tangent_policy(K, i["d_params"], i["d_pre"], i["d_actions"], i["d_x0"], i["d_v0"], mem.kind, o["hist"],
                                        o["d_obs"], o["d_pre"], o["d_actions"], o["d_x"], o["d_v"], o["d_E_mesh"])
        return self._tape_pass("tangent_policy", "tangent", mem, base, given, outs, call, K, batched, bump=True,
                               energies=("dKE", "dPE", "dPE_reward"))

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
        K, batched = directions("kl_smooth_jvp", {"d_x": (E, N), "d_v": (E, N)}, {"d_x": d_x, "d_v": d_v})
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
        K, batched = directions("moments_jvp", {"d_x": (E, N), "d_v": (E, N)}, {"d_x": d_x, "d_v": d_v})
        mem = Mem.of(self, d_x, d_v)
        tx, tv = mem.f64(d_x), mem.f64(d_v)
        out = mem.empty((K, E, 3, self.N_mesh))
        mem.enter()
        self._h.moments_jvp(K, mem.addr(tx), mem.addr(tv), mem.kind, mem.addr(out))
        return out if batched else out[0]

    # -- pooled particle features (pic_pool*; pic_pool_ln*, 7s) -----------------------------
    def _pool_call(self, who, W, b, activation, v_scale, x, v, on_device, cot=None, gamma=None, beta=None, eps=1e-5, period=None,
                   then=None):
        """The memory, the spec and the arrays of one pool call; every shape is checked here, before the device is touched.
        With gamma and beta the spec is pic_pool_ln's and the parameters are (W, b, gamma, beta).  `then`: the caller's own
        checks, run behind these and before the device is touched."""
        E, N = self.num_envs, self.N
        if activation not in _abi.ACTIVATIONS:
            raise ValueError(f"{who}: activation must be one of {sorted(_abi.ACTIVATIONS)}, not {activation!r}")
        ws, bs = tuple(np.shape(W)), tuple(np.shape(b))
        if len(ws) not in (2, 3) or ws[-1] != 3 or (len(ws) == 3 and ws[0] != E):
            raise ValueError(f"{who}: W must be [H, 3] or [num_envs, H, 3], not {list(ws)}")
        H, per_env = ws[-2], len(ws) == 3
        if not 1 <= H <= 256:
            raise ValueError(f"{who}: H must be 1..256, not {H}")
        if bs != ws[:-1]:
            raise ValueError(f"{who}: b must have shape {list(ws[:-1])}, not {list(bs)}")
        ln = gamma is not None or beta is not None
        if ln:
            if gamma is None or beta is None:
                raise ValueError(f"{who}: gamma and beta must both be given or both be None")
            for name, a in (("gamma", gamma), ("beta", beta)):
                if tuple(np.shape(a)) != bs:
                    raise ValueError(f"{who}: {name} must have shape {list(bs)}, not {list(np.shape(a))}")
            if not (np.isfinite(eps) and eps > 0):
                raise ValueError(f"{who}: eps must be finite and > 0, not {eps!r}")
            if period is not None and not (np.isfinite(period) and period >= 0):
                raise ValueError(f"{who}: period must be finite and >= 0 (0 or None: the environment's L), not {period!r}")
        if (x is None) != (v is None):
            raise ValueError(f"{who}: x and v must both be given or both be None")
        for name, a in (("x", x), ("v", v)):
            if a is not None and tuple(np.shape(a)) != (E, N):
                raise ValueError(f"{who}: {name} must be [num_envs, N] = {[E, N]}, not {list(np.shape(a))}")
        if cot is not None and tuple(np.shape(cot)) != (E, H):
            raise ValueError(f"{who}: cot must be [num_envs, H] = {[E, H]}, not {list(np.shape(cot))}")
        if not np.isfinite(v_scale):
            raise ValueError(f"{who}: v_scale must be finite, not {v_scale!r}")
        if then is not None:
            then()
        mem = Mem.of(self, W, b, x, v, cot, gamma, beta, force_device=on_device)
        lead = (E,) if per_env else ()
        parts = [mem.f64(W).reshape(lead + (3 * H,)), mem.f64(b)] + ([mem.f64(gamma), mem.f64(beta)] if ln else [])
        if mem.on_device:
            import torch
            params = torch.cat(parts, dim=-1).contiguous()
        else:
            params = np.ascontiguousarray(np.concatenate(parts, axis=-1))
        if ln:
            spec = _abi.PicPoolLnSpec(H, _abi.ACTIVATIONS[activation], int(per_env), mem.kind, float(v_scale), float(eps),
                                      float(period or 0.0), mem.addr(params))
        else:
            spec = _abi.PicPoolSpec(H, _abi.ACTIVATIONS[activation], int(per_env), mem.kind, float(v_scale), mem.addr(params))
        return mem, spec, params, H, per_env, mem.f64(x), mem.f64(v)

    def pool(self, W, b, activation: str = "tanh", v_scale: float = 1.0, x=None, v=None, on_device: bool = False,
             gamma=None, beta=None, eps: float = 1e-5, period=None):
        """The pooled particle features [num_envs, H] (pic_pool): out_k = mean_i act(b_k + W_k0 cos q_i + W_k1 sin q_i +
        W_k2 v_i v_scale), q = 2 pi x / L -- a DeepSets encoder's per-particle layer and mean without an [N, H] array.  W [H, 3]
        and b [H], or [num_envs, H, 3] and [num_envs, H] for per-environment parameters; x, v [num_envs, N] (positions need not
        be wrapped), or None: the stored particles of a float64 environment.  Bitwise reproducible and independent of the order
        of the particles.  NumPy, or float64 CUDA tensors if an input is one or with on_device.  The state is not touched.
        With gamma and beta (shaped like b) the layer is Linear -> LayerNorm(H; eps) -> act (pic_pool_ln): the
        pre-activations of each particle are normalised over the H units, scaled by gamma and shifted by beta; period (None or
        0: the environment's L) replaces L in q."""
        mem, spec, keep, H, _, x, v = self._pool_call("pool", W, b, activation, v_scale, x, v, on_device, None, gamma, beta, eps, period)
        out = mem.empty((self.num_envs, H))
        mem.enter()
        call = self._h.pool_ln if gamma is not None else self._h.pool
        call(spec, mem.addr(x), mem.addr(v), mem.kind, mem.addr(out))
        mem.leave(self._h)
        del keep
        return out

    def pool_vjp(self, W, b, cot, activation: str = "tanh", v_scale: float = 1.0, x=None, v=None, on_device: bool = False,
                 g_x: bool = True, g_v: bool = True, g_params: bool = True, gamma=None, beta=None, eps: float = 1e-5, period=None):
        """The vector-Jacobian product of `pool` for a cotangent cot [num_envs, H] (pic_pool_vjp) -> a dict: "g_x", "g_v"
        [num_envs, N], "g_W" and "g_b" shaped like W and b (shared parameters: summed over the environments in ascending
        order).  An output that is switched off (g_x, g_v, g_params = False) is None and is not computed.  With gamma and beta
        (pic_pool_ln_vjp) the dict also holds "g_gamma" and "g_beta", shaped like b."""
        if cot is None:
            raise ValueError("pool_vjp: cot must be [num_envs, H], not None")
        mem, spec, keep, H, per_env, x, v = self._pool_call("pool_vjp", W, b, activation, v_scale, x, v, on_device, cot, gamma, beta,
                                                            eps, period)
        E, N = self.num_envs, self.N
        ln = gamma is not None
        P = (6 if ln else 4) * H
        c = mem.f64(cot)
        gx = mem.empty((E, N)) if g_x else None
        gv = mem.empty((E, N)) if g_v else None
        gp = mem.empty((E, P) if per_env else (P,)) if g_params else None
        mem.enter()
        call = self._h.pool_ln_vjp if ln else self._h.pool_vjp
        call(spec, mem.addr(x), mem.addr(v), mem.addr(c), mem.kind, mem.addr(gx), mem.addr(gv), mem.addr(gp))
        mem.leave(self._h)
        del keep
        lead = (E,) if per_env else ()
        g = {"g_x": gx, "g_v": gv, "g_W": None if gp is None else gp[..., :3 * H].reshape(lead + (H, 3)),
             "g_b": None if gp is None else gp[..., 3 * H:4 * H]}
        if ln:
            g["g_gamma"] = None if gp is None else gp[..., 4 * H:5 * H]
            g["g_beta"] = None if gp is None else gp[..., 5 * H:]
        return g

    def pool_jvp(self, W, b, d_x=None, d_v=None, d_W=None, d_b=None, activation: str = "tanh", v_scale: float = 1.0, x=None, v=None,
                 on_device: bool = False, gamma=None, beta=None, d_gamma=None, d_beta=None, eps: float = 1e-5, period=None):
        """Directional derivatives of `pool` along tangents d_x, d_v [num_envs, N] of the particles and d_W, d_b (with gamma and
        beta: d_gamma, d_beta too) shaped like the parameters, each None = 0 (pic_pool_jvp, pic_pool_ln_jvp) ->
        [num_envs, H], dual to pool_vjp: sum cot . pool_jvp = g_x . d_x + g_v . d_v + g_W . d_W + ...  With a leading axis of
        K <= 8 directions on the tangents the result is [K, num_envs, H], bit for bit what K calls of one direction give.
        Bitwise reproducible and independent of the order of the particles.  NumPy, or a float64 CUDA tensor if an input is one
        or with on_device."""
        who = "pool_jvp"
        ln = gamma is not None or beta is not None
        if not ln and (d_gamma is not None or d_beta is not None):
            raise ValueError(f"{who}: d_gamma and d_beta need gamma and beta")
        given = {"d_x": d_x, "d_v": d_v, "d_W": d_W, "d_b": d_b, "d_gamma": d_gamma, "d_beta": d_beta}
        given = {k: a if a is None or hasattr(a, "shape") else np.asarray(a) for k, a in given.items()}
        dirs = []

        def check():
            ws, bs = tuple(np.shape(W)), tuple(np.shape(b))
            rows = (self.num_envs, self.N)
            dirs.append(directions(who, {"d_x": rows, "d_v": rows, "d_W": ws, "d_b": bs, "d_gamma": bs, "d_beta": bs}, given))

        # (a tangent that is a CUDA tensor moves the whole call to the device, as any other input does)
        on_device = on_device or any(getattr(a, "is_cuda", False) for a in given.values())
        mem, spec, keep, H, per_env, x, v = self._pool_call(who, W, b, activation, v_scale, x, v, on_device, None, gamma, beta, eps,
                                                            period, then=check)
        K, batched = dirs[0]
        E, N = self.num_envs, self.N
        tx, tv = mem.f64(d_x, (K, E, N)), mem.f64(d_v, (K, E, N))
        names = ("d_W", "d_b") + (("d_gamma", "d_beta") if ln else ())
        tparams = None
        if any(given[k] is not None for k in names):
            lead = (K, E) if per_env else (K,)
            tparams = mem.zeros(lead + ((6 if ln else 4) * H,))
            for k, lo, n in zip(names, (0, 3 * H, 4 * H, 5 * H), (3 * H, H, H, H)):
                if given[k] is not None:
                    tparams[..., lo:lo + n] = mem.f64(given[k], lead + (n,))
        out = mem.empty((K, E, H))
        mem.enter()
        call = self._h.pool_ln_jvp if ln else self._h.pool_jvp
        call(spec, mem.addr(x), mem.addr(v), K, mem.addr(tx), mem.addr(tv), mem.addr(tparams), mem.kind, mem.addr(out))
        mem.leave(self._h)
        del keep
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


class TangentWalk:
    """A forward-mode walk over an open tape (BatchedPIC.tangent_walk)."""

    def __init__(self, env, K, obs_modes, d_x0=None, d_v0=None, d_gain=None, on_device=False):
        E, N, n = env.num_envs, env.N, 2 * env.max_mode
        base = {"d_x0": (E, N), "d_v0": (E, N), "d_gain": (E, n, n)}
        given = {"d_x0": d_x0, "d_v0": d_v0, "d_gain": d_gain}
        self.K, self.batched = directions("tangent_walk", base, given, K)
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
        given = {"d_actions": d_actions, "d_ext": d_ext}
        directions("tangent_walk.step", base, given, walk=(K, self.batched))
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
