"""Independent oracle of the forward mode: the tangent equations the device kernels implement, in NumPy on the
restatement of tests/hp_adjoint.py, and torch forward-mode AD of that restatement.

The tangent of a direction: dq_1 = dx + c1 dt dv, dp_0 = dv; per sub-stage k = 1..3 dF_k = K drho(q_k) + de_t,
dE_k = W(q_k) . dF_k + dq_k (F_k[jr] - F_k[j]) / dx, dp_k = dp_{k-1} - d_k dt dE_k, dq_{k+1} = dq_k + c_{k+1} dt dp_k; then
dx' = dq_4, dv' = dp_3, dM = K drho(x'), dKE = sum p_3 dp_3, dPE_reward = dx sum M dM, dPE = N/L dPE_reward.  The deposit is
drho_j = s sum_i W'_j(q_i) dq_i: -dq / dx to the left node and +dq / dx to the right one, times s."""
import numpy as np
import torch

import hp_adjoint as ha


def _tangent_deposit(dq, q, S):
    jl, jr, _, _ = ha._np_cic(q, S)
    return (np.bincount(jr, dq, S.Ng) - np.bincount(jl, dq, S.Ng)) * (S.scale / S.dx)


def hand_jvp(x0, v0, ext, S, d_ext=None, d_x0=None, d_v0=None):
    """The forward equations above: returns d_hist [T, 3] (KE, PE, PE_reward), dx_T, dv_T [N] and dE_mesh [T, Ng]."""
    T = ext.shape[0]
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    dx = np.zeros(S.N) if d_x0 is None else np.array(d_x0, dtype=np.float64)
    dv = np.zeros(S.N) if d_v0 is None else np.array(d_v0, dtype=np.float64)
    de_all = np.zeros((T, S.Ng)) if d_ext is None else np.asarray(d_ext, dtype=np.float64)
    hist, dM_all = np.zeros((T, 3)), np.zeros((T, S.Ng))
    for t in range(T):
        qs, ps, Fs, xn, M = ha._np_forward_step(x, v, ext[t], S)
        dq = dx + (ha.CS[0] * S.dt) * dv
        dp = dv
        for k in (1, 2, 3):
            q = qs[k - 1]
            dF = ha._np_K(_tangent_deposit(dq, q, S), S) + de_all[t]
            jl, jr, wl, wr = ha._np_cic(q, S)
            F = Fs[k - 1]
            dE = (wl * dF[jl] + wr * dF[jr]) + dq * (F[jr] - F[jl]) / S.dx
            dp = dp - ha.DS[k] * S.dt * dE
            dq = dq + ha.CS[k] * S.dt * dp
        dM = ha._np_K(_tangent_deposit(dq, xn, S), S)
        per = S.dx * float((M * dM).sum())
        hist[t] = (float((ps[3] * dp).sum()), S.N / S.L * per, per)
        dM_all[t] = dM
        x, v, dx, dv = xn, ps[3], dq, dp
    return hist, dx, dv, dM_all


def _trajectory(x0, v0, ext, S):
    x, v = x0, v0
    hist, Ms = [], []
    for t in range(ext.shape[0]):
        x, v, ke, pe, per, M = ha.step(x, v, ext[t], S)
        hist.append(torch.stack([ke, pe, per]))
        Ms.append(M)
    return torch.stack(hist), x, v, torch.stack(Ms)


def torch_jvp(x0, v0, ext, S, d_ext=None, d_x0=None, d_v0=None):
    """The same tangents by torch forward-mode AD of the restatement (torch.autograd.forward_ad)."""
    import torch.autograd.forward_ad as fwAD

    def t64(a):
        return torch.as_tensor(np.asarray(a, dtype=np.float64))
    z = np.zeros
    with fwAD.dual_level():
        xd = fwAD.make_dual(t64(x0), t64(z(S.N) if d_x0 is None else d_x0))
        vd = fwAD.make_dual(t64(v0), t64(z(S.N) if d_v0 is None else d_v0))
        ed = fwAD.make_dual(t64(ext), t64(z(ext.shape) if d_ext is None else d_ext))
        outs = _trajectory(xd, vd, ed, S)
        return tuple(fwAD.unpack_dual(o).tangent.numpy().copy() for o in outs)
