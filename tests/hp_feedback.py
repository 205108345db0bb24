"""Oracle of the gain law: the closed loop a_t = G m_t(E_t) restated in float64 torch on the CPU on top of the
Yoshida-4 step of tests/hp_adjoint.py and differentiated by autograd, plus the hand-written law terms of the reverse pass in
NumPy (what law_adjoint_kernel and adjoint_start_kernel compute).

m = (Re E_1..Re E_M, Im E_1..Im E_M) with E_m = fft(E_mesh)[m] / Ng * 2 (spectrum.py:16); the actuator field of a is
B a = bc a[:M] + bs a[M:] (actuator.py:54-63, oracle.pic_oracle.actuator_basis).
"""
import numpy as np
import torch

import hp_adjoint as ha
from oracle import pic_oracle as po


def g0(M):
    """The reference's law run_feedback.py:133-135 as a gain: diag(-1 x M, +1 x M)."""
    return np.diag(np.concatenate([-np.ones(M), np.ones(M)]))


def twiddles(Ng, M):
    j = np.arange(Ng)
    th = 2 * np.pi * np.outer(np.arange(1, M + 1), j) / Ng
    return np.cos(th), np.sin(th)                                   # [M, Ng] each


def jacobian(Ng, M):
    """J [2M, Ng]: m = J E (mesh_mode's linear map)."""
    c, s = twiddles(Ng, M)
    return np.concatenate([c, -s], axis=0) * (2.0 / Ng)


def basis(L, Ng, M):
    bc, bs = po.actuator_basis(L, Ng, M)
    return np.concatenate([bc, bs], axis=1)                         # B [Ng, 2M]


def law_action(G, m):
    """The device's product: non-zero G[i][k] in ascending k, the first term starting the sum (host loop of the header)."""
    n = len(m)
    a = np.zeros(n)
    for i in range(n):
        acc, anyt = 0.0, False
        for k in range(n):
            if G[i][k] != 0.0:
                t = float(G[i][k]) * float(m[k])
                acc = acc + t if anyt else t
                anyt = True
        a[i] = acc
    return a


def rollout(x0, v0, G, S, T, M, E0=None):
    """T closed-loop steps from (x0, v0) under a_t = G m_t.  E0: the field the first step reads (default: the field of x0).
    Returns x_T, v_T, hist [T, 3] (KE, PE, PE_reward), modes [T, 2M], actions [T, 2M]."""
    J = torch.as_tensor(jacobian(S.Ng, M))
    B = torch.as_tensor(basis(S.L, S.Ng, M))
    x, v = x0, v0
    Ecur = ha.field(ha.density(x0, S), S) if E0 is None else E0
    hist, modes, acts = [], [], []
    for _ in range(T):
        m = J @ Ecur
        a = G @ m
        x, v, ke, pe, per, Ecur = ha.step(x, v, B @ a, S)
        hist.append(torch.stack([ke, pe, per]))
        modes.append(m)
        acts.append(a)
    return x, v, torch.stack(hist), torch.stack(modes), torch.stack(acts)


def objective_terms(xT, vT, hist, modes, cot_hist, cot_modes=None, cot_x=None, cot_v=None):
    J = (hist * torch.as_tensor(np.asarray(cot_hist, dtype=np.float64))).sum()
    if cot_modes is not None:
        J = J + (modes * torch.as_tensor(np.asarray(cot_modes, dtype=np.float64))).sum()
    if cot_x is not None:
        J = J + (xT * torch.as_tensor(np.asarray(cot_x, dtype=np.float64))).sum()
    if cot_v is not None:
        J = J + (vT * torch.as_tensor(np.asarray(cot_v, dtype=np.float64))).sum()
    return J


def autograd_vjp(x0, v0, G, S, T, M, cot_hist, cot_modes=None, cot_x=None, cot_v=None):
    """Gradients (G [2M, 2M], x0 [N], v0 [N]) of <cot_hist, hist> + <cot_modes, modes> + <cot_x, x_T> + <cot_v, v_T>, by
    autograd; also the modes and actions of the rollout."""
    x0 = torch.as_tensor(np.asarray(x0, dtype=np.float64)).clone().requires_grad_(True)
    v0 = torch.as_tensor(np.asarray(v0, dtype=np.float64)).clone().requires_grad_(True)
    Gt = torch.as_tensor(np.asarray(G, dtype=np.float64)).clone().requires_grad_(True)
    xT, vT, hist, modes, acts = rollout(x0, v0, Gt, S, T, M)
    J = objective_terms(xT, vT, hist, modes, cot_hist, cot_modes, cot_x, cot_v)
    gG, gx, gv = torch.autograd.grad(J, (Gt, x0, v0))
    return gG.numpy(), gx.numpy(), gv.numpy(), modes.detach().numpy(), acts.detach().numpy()


def objective(x0, v0, G, S, T, M, cot_hist, cot_modes=None, cot_x=None, cot_v=None):
    with torch.no_grad():
        xT, vT, hist, modes, _ = rollout(torch.as_tensor(x0), torch.as_tensor(v0), torch.as_tensor(G), S, T, M)
        return float(objective_terms(xT, vT, hist, modes, cot_hist, cot_modes, cot_x, cot_v))


# ---- the law's terms of the reverse pass, NumPy -------------------------------------------------------------
def hand_law_terms(G, e_bar, cot_m, S, M):
    """a-bar = B^T e-bar, m-bar = G^T a-bar + cot_m, E-bar = J^T m-bar for one law step."""
    a_bar = basis(S.L, S.Ng, M).T @ e_bar
    m_bar = np.asarray(G).T @ a_bar + cot_m
    return a_bar, m_bar, jacobian(S.Ng, M).T @ m_bar


def hand_start_term(x0, E_bar0, S):
    """The x_0 part of a first law step: s W'(x_0) . K^T E-bar_0 (K^T = -K on mean-free meshes)."""
    nu = -ha._np_K(E_bar0, S)
    return S.scale * ha._slope(nu, np.asarray(x0, dtype=np.float64), S)
