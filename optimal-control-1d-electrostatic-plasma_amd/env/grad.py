"""Differentiable rollouts for torch: the energy traces of a rollout as functions of its actions (or raw external fields), with
the gradient from the device's adjoint (pic_tape_backward).

    KE, PE, PE_reward = rollout(env, actions)      # actions: float64 CUDA tensor [T, num_envs, 2*max_mode], requires_grad
    (PE_reward.sum() + lam * (actions ** 2).sum() * L / 4).backward()   # fills actions.grad

    KE, PE, PE_reward, modes = rollout_feedback(env, gain, T)   # gain: [num_envs, 2M, 2M] or [2M, 2M], requires_grad
    (PE_reward.sum() + (modes[..., 0] ** 2).sum()).backward()  # fills gain.grad through the closed loop

Each call opens a fresh tape on `env` (an open one is stopped first) and leaves it open for the backward; stop it with
`env.stop_tape()` before a reset.  A backward after the environment has moved on (a further step, another rollout, a reset)
raises PicError.
"""
import numpy as np
import torch

from .._abi import PicError


def _start(env, T, checkpoint_every):
    env.stop_tape()
    env.start_tape(T, checkpoint_every)
    env._tape_serial = getattr(env, "_tape_serial", 0) + 1
    return env._tape_serial


class _Rollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, env, kind, checkpoint_every):
        if not (u.dtype == torch.float64 and u.dim() == 3 and u.shape[1] == env.num_envs):
            raise ValueError("the control must be a float64 tensor [T, num_envs, ...]")
        T = int(u.shape[0])
        serial = _start(env, T, checkpoint_every)
        host = np.ascontiguousarray(u.detach().cpu().numpy())
        if kind == "actions":
            ke, pe, per = env.step_actions_traj(host, history=True)
        else:
            ke, pe, per = env.step_ext_traj(host, history=True)
        ctx.env, ctx.kind, ctx.serial, ctx.steps = env, kind, serial, T
        return tuple(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=u.device) for a in (ke, pe, per))

    @staticmethod
    def backward(ctx, g_ke, g_pe, g_per):
        env = ctx.env
        if getattr(env, "_tape_serial", None) != ctx.serial or env.tape_stats()["steps"] != ctx.steps:
            raise PicError("backward: the environment has moved on since this rollout (a further step, rollout or reset)")
        if g_ke.is_cuda:
            out = env.backward(d_KE=g_ke.contiguous(), d_PE=g_pe.contiguous(), d_PE_reward=g_per.contiguous())
            g = out["actions"] if ctx.kind == "actions" else out["ext"]
        else:
            out = env.backward(d_KE=g_ke.numpy(), d_PE=g_pe.numpy(), d_PE_reward=g_per.numpy())
            g = torch.as_tensor(out["actions"] if ctx.kind == "actions" else out["ext"])
        return g, None, None, None


def rollout(env, actions, checkpoint_every=0):
    """T = actions.shape[0] steps of `env` (a BatchedPIC with an actuator) under actions [T, num_envs, 2*max_mode] through
    pic_step_actions_traj on a tape; returns KE, PE, PE_reward [T, num_envs] (float64, on actions' device), differentiable
    with respect to `actions`."""
    if getattr(env, "max_mode", 0) == 0:
        raise PicError("rollout: the environment has no actuator (set_actuator)")
    return _Rollout.apply(actions, env, "actions", int(checkpoint_every))


def rollout_ext(env, E_ext, checkpoint_every=0):
    """The same under raw external fields E_ext [T, num_envs, N_mesh] (pic_step_ext_traj)."""
    return _Rollout.apply(E_ext, env, "ext", int(checkpoint_every))


class _RolloutFeedback(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gain, env, T, checkpoint_every):
        E, n = env.num_envs, 2 * env.max_mode
        if not (gain.dtype == torch.float64 and tuple(gain.shape) in ((E, n, n), (n, n))):
            raise ValueError(f"the gain must be a float64 tensor [{E}, {n}, {n}] or [{n}, {n}]")
        serial = _start(env, T, checkpoint_every)
        g = gain.detach()
        if not g.is_cuda:
            g = g.numpy()
        out = env.step_feedback_gain(g, T, modes=True, history=True)
        ctx.env, ctx.serial, ctx.steps, ctx.shared = env, serial, T, gain.dim() == 2
        return tuple(torch.as_tensor(np.ascontiguousarray(out[k]), dtype=torch.float64, device=gain.device)
                     for k in ("KE", "PE", "PE_reward", "modes"))

    @staticmethod
    def backward(ctx, g_ke, g_pe, g_per, g_modes):
        env = ctx.env
        if getattr(env, "_tape_serial", None) != ctx.serial or env.tape_stats()["steps"] != ctx.steps:
            raise PicError("backward: the environment has moved on since this rollout (a further step, rollout or reset)")
        if g_ke.is_cuda:
            out = env.backward(d_KE=g_ke.contiguous(), d_PE=g_pe.contiguous(), d_PE_reward=g_per.contiguous(),
                               d_modes=g_modes.contiguous())
            g = out["gain"]
        else:
            out = env.backward(d_KE=g_ke.numpy(), d_PE=g_pe.numpy(), d_PE_reward=g_per.numpy(), d_modes=g_modes.numpy())
            g = torch.as_tensor(out["gain"])
        return (g.sum(0) if ctx.shared else g), None, None, None


def rollout_feedback(env, gain, T, checkpoint_every=0):
    """T steps of `env` (a BatchedPIC with an actuator) under the closed-loop gain law a_t = G m_t (step_feedback_gain) on a
    tape; returns KE, PE, PE_reward [T, num_envs] and the modes m_t [T, num_envs, 2*max_mode] the law read, differentiable with
    respect to `gain` (float64, [num_envs, 2M, 2M], or [2M, 2M] shared by every environment: its gradient is the sum over
    them).  Cotangents on `modes` reach the plasma through d_modes, so spectral losses such as sum |E_1|^2 work too."""
    if getattr(env, "max_mode", 0) == 0:
        raise PicError("rollout_feedback: the environment has no actuator (set_actuator)")
    return _RolloutFeedback.apply(gain, env, int(T), int(checkpoint_every))
