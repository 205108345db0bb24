"""Independent oracle of forward mode through closed loops: the hand-written tangent equations in NumPy -- one step
of tests/hp_tangent.py's hand_jvp at a time, with the action tangent of a step formed from the field tangent the step before
left -- and torch forward-mode AD of the closed-loop restatements (tests/hp_feedback.py: rollout, tests/hp_policy.py: rollout).

The gain law: dm_t = J dE_t, da_t = G dm_t + dG m_t (+ an injection), de_t = B da_t; dE_0 = K drho(x_0; dx_0).  A policy
a = fn(params, o): da_t = (d fn / d params) d_params + (d fn / d o) do_t with do_t = J dE_t (modes) or (dx_t, dv_t) (state); the
JVPs of the two policies of hp_policy.py are written out below."""
import numpy as np
import torch

import hp_adjoint as ha
import hp_feedback as hf
import hp_tangent as ht


def node_distance(x0, v0, exts, S):
    """The smallest distance, in cells, of a sub-stage position of the rollout from a mesh node (the derivative is
    the almost-everywhere one, so a position on a node makes every reference ambiguous)."""
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    worst = np.inf
    for e in exts:
        qs, ps, _, xn, _ = ha._np_forward_step(x, v, e, S)
        for q in qs:
            c = np.mod(q, S.L) / S.dx
            worst = min(worst, float(np.abs(c - np.round(c)).min()))
        x, v = xn, ps[-1]
    return worst


def _start_field(x0, dx0, S):
    E0 = ha._np_K(ha._np_density(x0, S) - S.n0, S)
    return E0, ha._np_K(ht._tangent_deposit(dx0, x0, S), S)


def _one_step(x, v, e, S, de, dx, dv):
    """One step of hand_jvp and of the forward: (hist row, dx', dv', dM), (x', v', M, primal hist row)."""
    h, ndx, ndv, dM = ht.hand_jvp(x, v, e[None], S, de[None], dx, dv)
    _, ps, _, xn, M = ha._np_forward_step(x, v, e, S)
    per = 0.5 * float((M * M).sum()) * S.dx
    return (h[0], ndx, ndv, dM[0]), (xn, ps[-1], M, np.array([0.5 * float((ps[-1] ** 2).sum()), per * S.N / S.L, per]))


def hand_feedback_jvp(x0, v0, G, S, T, M, dG=None, d_x0=None, d_v0=None, d_actions=None):
    """The closed loop a_t = G m_t in forward mode.  Returns d_hist [T, 3], d_modes [T, 2M], d_actions [T, 2M] (the total applied),
    dx_T, dv_T [N], dE_mesh [T, Ng] and the primal external fields [T, Ng]."""
    J, B = hf.jacobian(S.Ng, M), hf.basis(S.L, S.Ng, M)
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    dx = np.zeros(S.N) if d_x0 is None else np.array(d_x0, dtype=np.float64)
    dv = np.zeros(S.N) if d_v0 is None else np.array(d_v0, dtype=np.float64)
    dG = np.zeros_like(G) if dG is None else np.asarray(dG, dtype=np.float64)
    E, dE = _start_field(x, dx, S)
    hist, dms, das, dMs, exts = [], [], [], [], []
    for t in range(T):
        m, dm = J @ E, J @ dE
        da = G @ dm + dG @ m
        if d_actions is not None:
            da = da + d_actions[t]
        e = B @ (G @ m)
        (h, dx, dv, dE), (x, v, E, _) = _one_step(x, v, e, S, B @ da, dx, dv)
        hist.append(h), dms.append(dm), das.append(da), dMs.append(dE), exts.append(e)
    return np.stack(hist), np.stack(dms), np.stack(das), dx, dv, np.stack(dMs), np.stack(exts)


# ---- the policies of hp_policy.py and their JVPs, NumPy (one environment: no leading axes) -----------------------------------
def mlp_modes_np(p, m):
    return p["W2"] @ np.tanh(p["W1"] @ m + p["b1"]) + p["b2"]


def mlp_modes_jvp(p, m, dp, dm):
    h = np.tanh(p["W1"] @ m + p["b1"])
    dh = (1 - h * h) * (dp["W1"] @ m + p["W1"] @ dm + dp["b1"])
    return dp["W2"] @ h + p["W2"] @ dh + dp["b2"]


def _deepsets_hidden(p, xv, L):
    x, v = xv
    q = 2 * np.pi * x / L
    f = np.stack([np.cos(q), np.sin(q), v], axis=-1)
    return q, f, np.tanh(f @ p["W1"].T + p["b1"])


def deepsets_state_np(p, xv, L):
    return p["W2"] @ _deepsets_hidden(p, xv, L)[2].mean(0) + p["b2"]


def deepsets_state_jvp(p, xv, L, dp, dxv):
    q, f, h = _deepsets_hidden(p, xv, L)
    dq = 2 * np.pi * dxv[0] / L
    df = np.stack([-np.sin(q) * dq, np.cos(q) * dq, dxv[1]], axis=-1)
    dh = (1 - h * h) * (df @ p["W1"].T + f @ dp["W1"].T + dp["b1"])
    return dp["W2"] @ h.mean(0) + p["W2"] @ dh.mean(0) + dp["b2"]


def hand_policy_jvp(x0, v0, fn, fn_jvp, p, dp, S, T, M, observe="modes", obs_modes=None, d_x0=None, d_v0=None):
    """The closed loop a_t = fn(p, o_t) in forward mode, fn_jvp(p, o, dp, do) its JVP.  Returns d_hist [T, 3], d_actions [T, 2M],
    dx_T, dv_T and the primal external fields [T, Ng]."""
    Mo = M if obs_modes is None else int(obs_modes)
    J, B = hf.jacobian(S.Ng, Mo), hf.basis(S.L, S.Ng, M)
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    dx = np.zeros(S.N) if d_x0 is None else np.array(d_x0, dtype=np.float64)
    dv = np.zeros(S.N) if d_v0 is None else np.array(d_v0, dtype=np.float64)
    E, dE = _start_field(x, dx, S)
    hist, das, exts = [], [], []
    for t in range(T):
        o, do = (J @ E, J @ dE) if observe == "modes" else ((x, v), (dx, dv))
        a, da = fn(p, o), fn_jvp(p, o, dp, do)
        e = B @ a
        (h, dx, dv, dE), (x, v, E, _) = _one_step(x, v, e, S, B @ da, dx, dv)
        hist.append(h), das.append(da), exts.append(e)
    return np.stack(hist), np.stack(das), dx, dv, np.stack(exts)


# ---- torch forward mode of the restatements -------------------------------------------------------------------------------------
def _t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _tan(o):
    import torch.autograd.forward_ad as fwAD
    t = fwAD.unpack_dual(o).tangent
    return (torch.zeros_like(o) if t is None else t).numpy().copy()


def torch_feedback_jvp(x0, v0, G, S, T, M, dG=None, d_x0=None, d_v0=None):
    """Forward-mode AD of hp_feedback.rollout: d_hist [T, 3], d_modes [T, 2M], d_actions [T, 2M], dx_T, dv_T."""
    import torch.autograd.forward_ad as fwAD
    z = np.zeros
    with fwAD.dual_level():
        xd = fwAD.make_dual(_t64(x0), _t64(z(S.N) if d_x0 is None else d_x0))
        vd = fwAD.make_dual(_t64(v0), _t64(z(S.N) if d_v0 is None else d_v0))
        Gd = fwAD.make_dual(_t64(G), _t64(z(np.shape(G)) if dG is None else dG))
        xT, vT, hist, modes, acts = hf.rollout(xd, vd, Gd, S, T, M)
        return _tan(hist), _tan(modes), _tan(acts), _tan(xT), _tan(vT)


def torch_policy_jvp(x0, v0, fn, p, dp, S, T, M, observe="modes", obs_modes=None, d_x0=None, d_v0=None):
    """Forward-mode AD of hp_policy.rollout under the torch policy fn(params, o): d_hist [T, 3], d_actions [T, 2M]."""
    import torch.autograd.forward_ad as fwAD
    import hp_policy as hpol
    z = np.zeros
    with fwAD.dual_level():
        xd = fwAD.make_dual(_t64(x0), _t64(z(S.N) if d_x0 is None else d_x0))
        vd = fwAD.make_dual(_t64(v0), _t64(z(S.N) if d_v0 is None else d_v0))
        pd = {k: fwAD.make_dual(_t64(a), _t64(dp[k])) for k, a in p.items()}
        hist, acts, _ = hpol.rollout(xd, vd, lambda o: fn(pd, o), S, T, M, observe, obs_modes)
        return _tan(hist), _tan(acts)
