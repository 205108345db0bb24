"""Independent oracle of the adjoint: the Yoshida-4 step restated in float64 torch on the CPU and differentiated by
autograd, plus the hand-written reverse equations in NumPy that the device kernels implement.

Restatement of pic.py:131-146 for one environment:
  CIC with the reference's floor rule through scatter_add (interpolate.py:6-18), a mean-free periodic solve by FFT with the
  3-point Laplacian and the central difference (the operator the device's two scans compute), the gather, the four drifts and
  three kicks of integration.py:60-75, and KE, PE, PE_reward (util.py:119-147, objective.py:33).
"""
import math

import numpy as np
import torch

C1 = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
W0 = -(2.0 ** (1.0 / 3.0)) / (2.0 - 2.0 ** (1.0 / 3.0))
CS = (0.5 * C1, 0.5 * (W0 + C1), 0.5 * (W0 + C1), 0.5 * C1)
DS = (0.0, C1, W0, C1)


class Setup:
    def __init__(self, N, Ng, L=50.0, n0=1.0, dt=0.1):
        self.N, self.Ng, self.L, self.n0, self.dt = int(N), int(Ng), float(L), float(n0), float(dt)
        self.dx = self.L / self.Ng
        self.scale = self.n0 * self.L / self.N / self.dx
        k = np.arange(self.Ng)
        th = 2 * np.pi * k / self.Ng
        lam = (2 * np.cos(th) - 2) / self.dx ** 2
        with np.errstate(divide="ignore"):
            inv = np.where(k == 0, 0.0, 1.0 / np.where(k == 0, 1.0, lam))
        # E_hat = -(e^{i th} - e^{-i th}) / (2 dx) phi_hat = -i sin(th) / dx * b_hat / lam
        self.kop = torch.as_tensor(-1j * np.sin(th) / self.dx * inv, dtype=torch.complex128)


def cic(q, S):
    """Wrapped positions, left / right nodes and weights (interpolate.py:6-13)."""
    xw = torch.remainder(q, S.L)
    j = torch.floor((xw / S.dx).detach())
    wl = ((j + 1) * S.dx - xw) / S.dx
    wr = (xw - j * S.dx) / S.dx
    jl = j.long() % S.Ng
    jr = (jl + 1) % S.Ng
    return jl, jr, wl, wr


def density(q, S):
    jl, jr, wl, wr = cic(q, S)
    n = torch.zeros(S.Ng, dtype=torch.float64).scatter_add(0, jl, wl).scatter_add(0, jr, wr)
    return n * S.scale


def field(n, S):
    """E_mesh of the density n (no external field): K (n - n0)."""
    b = n - S.n0
    return torch.fft.ifft(torch.fft.fft(b - b.mean()) * S.kop).real


def gather(F, q, S):
    jl, jr, wl, wr = cic(q, S)
    return wl * F[jl] + wr * F[jr]


def step(x, v, e, S):
    """One Yoshida-4 step under the external mesh field e; returns x', v', KE, PE, PE_reward, E_mesh after the step."""
    q = x + CS[0] * v * S.dt
    p = v
    for k in (1, 2, 3):
        F = field(density(q, S), S) + e
        p = p + DS[k] * (-gather(F, q, S)) * S.dt
        q = q + CS[k] * p * S.dt
    xn = torch.remainder(q, S.L)
    M = field(density(xn, S), S)
    ke = 0.5 * (p * p).sum()
    per = 0.5 * (M * M).sum() * S.dx
    return xn, p, ke, per * S.N / S.L, per, M


def rollout(x0, v0, ext, S):
    """T steps; ext [T, Ng].  Returns x_T, v_T and the energy history [T, 3] (KE, PE, PE_reward)."""
    x, v = x0, v0
    hist = []
    for t in range(ext.shape[0]):
        x, v, ke, pe, per, _ = step(x, v, ext[t], S)
        hist.append(torch.stack([ke, pe, per]))
    return x, v, torch.stack(hist)


def autograd_vjp(x0, v0, ext, S, cot_hist, cot_x=None, cot_v=None):
    """Gradients (ext [T, Ng], x0 [N], v0 [N]) of <cot_hist, hist> + <cot_x, x_T> + <cot_v, v_T>, by autograd."""
    x0 = torch.as_tensor(np.asarray(x0, dtype=np.float64)).clone().requires_grad_(True)
    v0 = torch.as_tensor(np.asarray(v0, dtype=np.float64)).clone().requires_grad_(True)
    e = torch.as_tensor(np.asarray(ext, dtype=np.float64)).clone().requires_grad_(True)
    xT, vT, hist = rollout(x0, v0, e, S)
    J = (hist * torch.as_tensor(np.asarray(cot_hist, dtype=np.float64))).sum()
    if cot_x is not None:
        J = J + (xT * torch.as_tensor(np.asarray(cot_x, dtype=np.float64))).sum()
    if cot_v is not None:
        J = J + (vT * torch.as_tensor(np.asarray(cot_v, dtype=np.float64))).sum()
    ge, gx, gv = torch.autograd.grad(J, (e, x0, v0))
    return ge.numpy(), gx.numpy(), gv.numpy()


def objective(x0, v0, ext, S, cot_hist, cot_x=None, cot_v=None):
    with torch.no_grad():
        xT, vT, hist = rollout(torch.as_tensor(x0), torch.as_tensor(v0), torch.as_tensor(ext), S)
        J = float((hist * torch.as_tensor(cot_hist)).sum())
        if cot_x is not None:
            J += float((xT * torch.as_tensor(cot_x)).sum())
        if cot_v is not None:
            J += float((vT * torch.as_tensor(cot_v)).sum())
    return J


# ---- the hand-written reverse pass, NumPy ------------------------------------------------------------------
def _np_cic(q, S):
    xw = np.mod(q, S.L)
    j = np.floor(xw / S.dx)
    wl = ((j + 1) * S.dx - xw) / S.dx
    wr = (xw - j * S.dx) / S.dx
    jl = j.astype(np.int64) % S.Ng
    return jl, (jl + 1) % S.Ng, wl, wr


def _np_K(b, S):
    """E = K b for a mesh b (mean removed first)."""
    return np.fft.ifft(np.fft.fft(b - b.mean()) * S.kop.numpy()).real


def _np_density(q, S):
    jl, jr, wl, wr = _np_cic(q, S)
    return (np.bincount(jl, wl, S.Ng) + np.bincount(jr, wr, S.Ng)) * S.scale


def _np_forward_step(x, v, e, S):
    qs, ps, Fs = [x + CS[0] * v * S.dt], [v], []
    for k in (1, 2, 3):
        F = _np_K(_np_density(qs[-1], S) - S.n0, S) + e
        jl, jr, wl, wr = _np_cic(qs[-1], S)
        ps.append(ps[-1] + DS[k] * (-(wl * F[jl] + wr * F[jr])) * S.dt)
        qs.append(qs[-1] + CS[k] * ps[-1] * S.dt)
        Fs.append(F)
    xn = np.mod(qs[-1], S.L)
    M = _np_K(_np_density(xn, S) - S.n0, S)
    return qs, ps, Fs, xn, M


def _slope(m, q, S):
    jl, jr, _, _ = _np_cic(q, S)
    return (m[jr] - m[jl]) / S.dx


def _deposit(c, q, S):
    jl, jr, wl, wr = _np_cic(q, S)
    return np.bincount(jl, c * wl, S.Ng) + np.bincount(jr, c * wr, S.Ng)


def hand_vjp(x0, v0, ext, S, cot_hist, cot_x=None, cot_v=None):
    """The reverse equations of DESIGN.md 7c (what adjoint_pass / deposit / mesh kernels compute), with the forward states
    stored instead of replayed."""
    T = ext.shape[0]
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    tape = []
    for t in range(T):
        qs, ps, Fs, xn, M = _np_forward_step(x, v, ext[t], S)
        tape.append((qs, ps, Fs, xn, M))
        x, v = xn, ps[-1]
    lx = np.zeros(S.N) if cot_x is None else np.array(cot_x, dtype=np.float64)
    lv = np.zeros(S.N) if cot_v is None else np.array(cot_v, dtype=np.float64)
    ge = np.zeros((T, S.Ng))
    for t in range(T - 1, -1, -1):
        qs, ps, Fs, xn, M = tape[t]
        a_ke, a_pe, a_per = cot_hist[t]
        lv = lv + a_ke * ps[3]
        m = (a_pe * S.N / S.L + a_per) * S.dx * M
        nu = -_np_K(m, S)
        lx = lx + S.scale * _slope(nu, xn, S)
        lq = lx
        lp = lv + CS[3] * S.dt * lq
        for k in (3, 2, 1):
            c = -DS[k] * S.dt * lp
            mu = _deposit(c, qs[k - 1], S)
            ge[t] += mu
            nu = -_np_K(mu, S)
            lq = lq + c * _slope(Fs[k - 1], qs[k - 1], S) + S.scale * _slope(nu, qs[k - 1], S)
            lp = lp + CS[k - 1] * S.dt * lq
        lx, lv = lq, lp
    return ge, lx, lv
