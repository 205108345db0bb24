"""Independent oracle of the forward mode of the per-step smoothed KL: hp_tangent's tangent equations with, behind
every step t, the dot product of the KL's gradient at the state the step left with the tangent of that state,

    dKL~_t = <dKL~/dx', dx'> + <dKL~/dv', dv'>,   (dKL~/dx', dKL~/dv') = hp_phase.vjp(x', v', d_kl = 1),   (dx', dv') = (dq_4, dp_3)

in NumPy, and torch forward-mode AD of hp_tape_kl.rollout (the straight-through density: the device's values, the derivative of
the unquantised weights).  One environment: x0, v0 [N], ext [T, Ng], feq [nx, nv]; S a hp_adjoint.Setup, G a hp_phase.Grid."""
import numpy as np
import torch

import hp_adjoint as ha
import hp_phase as hp
import hp_tangent as ht
import hp_tape_kl as hk


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def hand_jvp(x0, v0, ext, S, G, feq, d_ext=None, d_x0=None, d_v0=None):
    """hp_tangent.hand_jvp's step with the KL's dot product behind it: returns d_hist [T, 3] (KE, PE, PE_reward), d_kl [T] and
    dx_T, dv_T [N]."""
    T = ext.shape[0]
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    dx = np.zeros(S.N) if d_x0 is None else np.array(d_x0, dtype=np.float64)
    dv = np.zeros(S.N) if d_v0 is None else np.array(d_v0, dtype=np.float64)
    de_all = np.zeros((T, S.Ng)) if d_ext is None else np.asarray(d_ext, dtype=np.float64)
    hist, dkl = np.zeros((T, 3)), np.zeros(T)
    one = _t([1.0])
    for t in range(T):
        qs, ps, Fs, xn, M = ha._np_forward_step(x, v, ext[t], S)
        dq = dx + (ha.CS[0] * S.dt) * dv
        dp = dv
        for k in (1, 2, 3):
            q = qs[k - 1]
            dF = ha._np_K(ht._tangent_deposit(dq, q, S), S) + de_all[t]
            jl, jr, wl, wr = ha._np_cic(q, S)
            F = Fs[k - 1]
            dE = (wl * dF[jl] + wr * dF[jr]) + dq * (F[jr] - F[jl]) / S.dx
            dp = dp - ha.DS[k] * S.dt * dE
            dq = dq + ha.CS[k] * S.dt * dp
        gx, gv = hp.vjp(_t(xn)[None], _t(ps[3])[None], _t(feq), one, G)
        dkl[t] = float((gx[0].numpy() * dq).sum() + (gv[0].numpy() * dp).sum())
        dM = ha._np_K(ht._tangent_deposit(dq, xn, S), S)
        per = S.dx * float((M * dM).sum())
        hist[t] = (float((ps[3] * dp).sum()), S.N / S.L * per, per)
        x, v, dx, dv = xn, ps[3], dq, dp
    return hist, dkl, dx, dv


def torch_jvp(x0, v0, ext, S, G, feq, d_ext=None, d_x0=None, d_v0=None):
    """The same tangents by torch forward-mode AD of hp_tape_kl.rollout: d_hist [T, 3], d_kl [T], dx_T, dv_T [N]."""
    import torch.autograd.forward_ad as fwAD
    z = np.zeros
    with fwAD.dual_level():
        xd = fwAD.make_dual(_t(x0), _t(z(S.N) if d_x0 is None else d_x0))
        vd = fwAD.make_dual(_t(v0), _t(z(S.N) if d_v0 is None else d_v0))
        ed = fwAD.make_dual(_t(ext), _t(z(ext.shape) if d_ext is None else d_ext))
        xT, vT, hist, kls = hk.rollout(xd, vd, ed, S, G, _t(feq))

        def tan(o):
            t = fwAD.unpack_dual(o).tangent
            return np.zeros(tuple(o.shape)) if t is None else t.numpy().copy()
        return tan(hist), tan(kls), tan(xT), tan(vT)
