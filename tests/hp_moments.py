"""Independent restatement of the fluid moments on the mesh.  TEST INFRASTRUCTURE ONLY.

    m0_j = s sum_i W_j(x_i)      m1_j = s sum_i W_j(x_i) v_i      m2_j = s sum_i W_j(x_i) v_i^2      s = n0 L / (N dx)

* `moments_ld`: np.longdouble, from particles as the device holds them, with the cells and exact weights of
  tests/hp_reference.py (CIC with the reference's floor rule, TSC as hp_reference.deposit) accumulated by np.add.at
  (np.bincount would cast the weights to float64);
* `moments_torch`: the same in float64 torch with the floor detached (hp_adjoint.cic), for autograd;
* `hand_vjp`: the gather the device implements, in NumPy;
* `rollout_moments` / `rollout_policy`: hp_adjoint.step with the moments of every state, open loop under given fields or in
  closed loop under a policy that observes them.
"""
import numpy as np
import torch

import hp_adjoint as ha
import hp_feedback as hf
import hp_reference as hr

LD = hr.LD


def moments_ld(x, v, Ng, L, n0=1.0, shape="CIC", cell_dtype=None):
    """[3, Ng] longdouble from one environment's particles (x: lengths or uint32 fixed point; v any float dtype)."""
    x = np.asarray(x)
    N = x.shape[0]
    jf, d = hr._cells(x, Ng, L, cell_dtype)
    offs, w = hr.shape_weights(d, shape)
    vl = hr.as_ld(v)
    m = np.zeros((3, Ng), dtype=LD)
    for o, wk in zip(offs, w):
        nodes = np.mod(jf + o, Ng)
        np.add.at(m[0], nodes, wk)
        np.add.at(m[1], nodes, wk * vl)
        np.add.at(m[2], nodes, wk * vl * vl)
    dx = LD(L) / LD(Ng)
    return m * (LD(n0) * LD(L) / LD(N) / dx)


def moments_torch(x, v, S):
    """[3, Ng] float64 torch, differentiable in x and v (the floor of the cell index detached)."""
    jl, jr, wl, wr = ha.cic(x, S)
    z = torch.zeros(S.Ng, dtype=torch.float64)
    rows = [z.scatter_add(0, jl, wl * f).scatter_add(0, jr, wr * f) for f in (torch.ones_like(v), v, v * v)]
    return torch.stack(rows) * S.scale


def autograd_vjp(x, v, g, S):
    """(g_x, g_v) of <g, moments(x, v)> by autograd; g [3, Ng]."""
    xt = torch.as_tensor(np.asarray(x, dtype=np.float64)).clone().requires_grad_(True)
    vt = torch.as_tensor(np.asarray(v, dtype=np.float64)).clone().requires_grad_(True)
    J = (moments_torch(xt, vt, S) * torch.as_tensor(np.asarray(g, dtype=np.float64))).sum()
    gx, gv = torch.autograd.grad(J, (xt, vt))
    return gx.numpy(), gv.numpy()


def hand_vjp(x, v, g, S):
    """The gather of include/picstep.h: pic_moments_vjp, in NumPy float64."""
    x, v, g = (np.asarray(a, dtype=np.float64) for a in (x, v, g))
    jl, jr, wl, wr = ha._np_cic(x, S)
    slope = lambda c: (c[jr] - c[jl]) / S.dx  # noqa: E731
    gx = S.scale * (slope(g[0]) + v * slope(g[1]) + v * v * slope(g[2]))
    gv = S.scale * ((wl * g[1][jl] + wr * g[1][jr]) + 2.0 * v * (wl * g[2][jl] + wr * g[2][jr]))
    return gx, gv


def rollout_moments(x0, v0, ext, S):
    """T open-loop steps under ext [T, Ng]: x_T, v_T, the energy history [T, 3], the moments of the states the steps left
    [T, 3, Ng] and those of the starting state [3, Ng]."""
    x, v = x0, v0
    hist, mom = [], []
    for t in range(ext.shape[0]):
        x, v, ke, pe, per, _ = ha.step(x, v, ext[t], S)
        hist.append(torch.stack([ke, pe, per]))
        mom.append(moments_torch(x, v, S))
    return x, v, torch.stack(hist), torch.stack(mom), moments_torch(x0, v0, S)


def rollout_policy(x0, v0, policy, S, T, M):
    """T closed-loop steps of one environment under a_t = policy(o_t), o_t = the moments [3, Ng] of the state step t starts
    from.  Returns hist [T, 3] (KE, PE, PE_reward), actions [T, 2M] and o_0..o_T."""
    B = torch.as_tensor(hf.basis(S.L, S.Ng, M))
    x, v = x0, v0
    obs = [moments_torch(x, v, S)]
    hist, acts = [], []
    for _ in range(T):
        a = policy(obs[-1]).to(torch.float64)
        x, v, ke, pe, per, _ = ha.step(x, v, B @ a, S)
        hist.append(torch.stack([ke, pe, per]))
        acts.append(a)
        obs.append(moments_torch(x, v, S))
    return torch.stack(hist), torch.stack(acts), obs


def pool(o, width=8):
    """[..., 3, Ng] -> [..., 3 Ng / width]: the mean over `width` consecutive nodes of every moment."""
    return o.reshape(*o.shape[:-1], o.shape[-1] // width, width).mean(-1).flatten(-2)


def pooled_tanh_policy(W, width=8):
    """o -> tanh(pool(o) @ W): W [3 Ng / width, 2M], or with leading environment axes [E, 3 Ng / width, 2M] for o [E, 3, Ng]."""
    return lambda o: torch.tanh(torch.einsum("...i,...ia->...a", pool(o, width), W))
