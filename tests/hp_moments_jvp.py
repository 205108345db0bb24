"""Independent restatement of the forward mode of the fluid moments.  TEST INFRASTRUCTURE ONLY.

With j, jr the nodes and w_l, w_r the CIC weights of particle i, iota_i = dx_i / dx and s = n0 L / (N dx), particle i adds

    dm0:  -iota                      +iota
    dm1:  w_l dv - iota v            w_r dv + iota v
    dm2:  2 w_l v dv - iota v^2      2 w_r v dv + iota v^2

to its left and right node (times s): the transpose of hp_moments.hand_vjp, term by term.

* `hand_jvp`: the table in NumPy float64, one state;
* `jvp_ld`: the same in np.longdouble with the cells and exact weights of tests/hp_reference.py, from particles as the device
  holds them;
* `torch_jvp`: torch forward-mode AD of hp_moments.moments_torch;
* `rollout_hand_jvp`: the tangents of the moments of every state of a rollout, on hp_tangent.hand_jvp's per-step (dx', dv');
* `rollout_torch_jvp`: torch forward-mode AD of hp_moments.rollout_moments.
"""
import numpy as np
import torch

import hp_adjoint as ha
import hp_moments as hm
import hp_reference as hr
import hp_tangent as ht

LD = hr.LD


def _zeros_like_if_none(a, ref, dtype):
    return np.zeros(np.shape(ref), dtype=dtype) if a is None else np.asarray(a).astype(dtype)


def hand_jvp(x, v, d_x, d_v, S):
    """[3, Ng] float64: the tangent of hp_moments.moments_torch at (x, v) along (d_x, d_v) (each None = 0)."""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    dxs, dvs = _zeros_like_if_none(d_x, x, np.float64), _zeros_like_if_none(d_v, x, np.float64)
    jl, jr, wl, wr = ha._np_cic(x, S)
    io = dxs / S.dx
    left = (-io, wl * dvs - io * v, 2.0 * wl * v * dvs - io * v * v)
    right = (io, wr * dvs + io * v, 2.0 * wr * v * dvs + io * v * v)
    m = np.stack([np.bincount(jl, a, S.Ng) + np.bincount(jr, b, S.Ng) for a, b in zip(left, right)])
    return m * S.scale


def jvp_ld(x, v, d_x, d_v, Ng, L, n0=1.0, cell_dtype=np.float64):
    """[3, Ng] longdouble from one environment's float64 particles as the device holds them (the forward's float64 cell)."""
    x = np.asarray(x)
    N = x.shape[0]
    jf, d = hr._cells(x, Ng, L, cell_dtype)
    vl = hr.as_ld(v)
    dxs, dvs = _zeros_like_if_none(d_x, x, LD), _zeros_like_if_none(d_v, x, LD)
    dx = LD(L) / LD(Ng)
    io = dxs / dx
    wl, wr = 1 - d, d
    jl, jr = np.mod(jf, Ng), np.mod(jf + 1, Ng)
    m = np.zeros((3, Ng), dtype=LD)
    for k, (a, b) in enumerate(((-io, io), (wl * dvs - io * vl, wr * dvs + io * vl),
                                (2 * wl * vl * dvs - io * vl * vl, 2 * wr * vl * dvs + io * vl * vl))):
        np.add.at(m[k], jl, a)
        np.add.at(m[k], jr, b)
    return m * (LD(n0) * LD(L) / LD(N) / dx)


def torch_jvp(x, v, d_x, d_v, S):
    """[3, Ng] float64 by torch forward-mode AD of hp_moments.moments_torch."""
    import torch.autograd.forward_ad as fwAD
    t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    z = np.zeros(np.shape(x))
    with fwAD.dual_level():
        xd = fwAD.make_dual(t64(x), t64(z if d_x is None else d_x))
        vd = fwAD.make_dual(t64(v), t64(z if d_v is None else d_v))
        return fwAD.unpack_dual(hm.moments_torch(xd, vd, S)).tangent.numpy().copy()


def rollout_hand_jvp(x0, v0, ext, S, d_ext=None, d_x0=None, d_v0=None):
    """[T, 3, Ng]: the tangents of the moments of the state every step left, one step of hp_tangent.hand_jvp at a time."""
    T = ext.shape[0]
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    dxs, dvs = _zeros_like_if_none(d_x0, x, np.float64), _zeros_like_if_none(d_v0, x, np.float64)
    out = np.zeros((T, 3, S.Ng))
    for t in range(T):
        de = None if d_ext is None else np.asarray(d_ext, dtype=np.float64)[t:t + 1]
        _, dxs, dvs, _ = ht.hand_jvp(x, v, ext[t:t + 1], S, d_ext=de, d_x0=dxs, d_v0=dvs)
        _, ps, _, x, _ = ha._np_forward_step(x, v, ext[t], S)
        v = ps[3]
        out[t] = hand_jvp(x, v, dxs, dvs, S)
    return out


def rollout_torch_jvp(x0, v0, ext, S, d_ext=None, d_x0=None, d_v0=None):
    """[T, 3, Ng] by torch forward-mode AD of hp_moments.rollout_moments (the torch oracle of the tape's tangents)."""
    import torch.autograd.forward_ad as fwAD
    t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    z = np.zeros
    with fwAD.dual_level():
        xd = fwAD.make_dual(t64(x0), t64(z(S.N) if d_x0 is None else d_x0))
        vd = fwAD.make_dual(t64(v0), t64(z(S.N) if d_v0 is None else d_v0))
        ed = fwAD.make_dual(t64(ext), t64(z(np.shape(ext)) if d_ext is None else d_ext))
        mom = hm.rollout_moments(xd, vd, ed, S)[3]
        return fwAD.unpack_dual(mom).tangent.numpy().copy()
