"""Restatement of the per-step smoothed KL of a taped rollout, for the tests: hp_adjoint's Yoshida-4 step composed
with hp_phase's straight-through density and KL (the device's values, the derivative of the unquantised weights, which autograd
can see), the KL trace of a rollout and its vector-Jacobian product by autograd, and the hand equations in NumPy: hp_adjoint's
reverse pass with hp_phase.vjp injected behind every step,

    lambda_x' += k-bar_t dKL~_t/dx',   lambda_v' += k-bar_t dKL~_t/dv'        (before the refresh adjoint of step t).

One environment: x0, v0 [N], ext [T, Ng], feq [nx, nv]; S a hp_adjoint.Setup, G a hp_phase.Grid."""
import numpy as np
import torch

import hp_adjoint as ha
import hp_phase as hp


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def rollout(x0, v0, ext, S, G, feq, density=hp.density_st):
    """T steps; returns x_T, v_T, the energy history [T, 3] and the KL trace [T] (KL~ of the state every step left)."""
    x, v = x0, v0
    hist, kls = [], []
    for t in range(ext.shape[0]):
        x, v, ke, pe, per, _ = ha.step(x, v, ext[t], S)
        hist.append(torch.stack([ke, pe, per]))
        kls.append(hp.kl(density(x[None], v[None], G), feq, G)[0])
    return x, v, torch.stack(hist), torch.stack(kls)


def kl_trace(x0, v0, ext, S, G, feq):
    with torch.no_grad():
        return rollout(_t(x0), _t(v0), _t(ext), S, G, _t(feq))[3].numpy()


def _objective(xT, vT, hist, kls, cot_kl, cot_hist, cot_x, cot_v):
    J = (kls * _t(cot_kl)).sum()
    if cot_hist is not None:
        J = J + (hist * _t(cot_hist)).sum()
    if cot_x is not None:
        J = J + (xT * _t(cot_x)).sum()
    if cot_v is not None:
        J = J + (vT * _t(cot_v)).sum()
    return J


def autograd_vjp(x0, v0, ext, S, G, feq, cot_kl, cot_hist=None, cot_x=None, cot_v=None):
    """Gradients (ext [T, Ng], x0 [N], v0 [N]) of <cot_kl, KL> + <cot_hist, hist> + <cot_x, x_T> + <cot_v, v_T>, by autograd."""
    x0, v0, e = (_t(a).clone().requires_grad_(True) for a in (x0, v0, ext))
    J = _objective(*rollout(x0, v0, e, S, G, _t(feq)), cot_kl, cot_hist, cot_x, cot_v)
    ge, gx, gv = torch.autograd.grad(J, (e, x0, v0))
    return ge.numpy(), gx.numpy(), gv.numpy()


def objective(x0, v0, ext, S, G, feq, cot_kl, cot_hist=None, cot_x=None, cot_v=None, density=hp.density_smooth):
    """The same scalar as a float.  density_smooth by default: finite differences of it carry no quantisation noise, and the
    derivative under test is that of the unquantised weights."""
    with torch.no_grad():
        return float(_objective(*rollout(_t(x0), _t(v0), _t(ext), S, G, _t(feq), density), cot_kl, cot_hist, cot_x, cot_v))


def hand_vjp(x0, v0, ext, S, G, feq, cot_kl, cot_hist=None, cot_x=None, cot_v=None):
    """The reverse equations the device runs (DESIGN.md 7c with 7h's injection): hp_adjoint.hand_vjp's pass, and behind every
    step t the gather of hp_phase.vjp at the state it left, scaled by cot_kl[t]."""
    T = ext.shape[0]
    if cot_hist is None:
        cot_hist = np.zeros((T, 3))
    x, v = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    tape = []
    for t in range(T):
        qs, ps, Fs, xn, M = ha._np_forward_step(x, v, ext[t], S)
        tape.append((qs, ps, Fs, xn, M))
        x, v = xn, ps[-1]
    lx = np.zeros(S.N) if cot_x is None else np.array(cot_x, dtype=np.float64)
    lv = np.zeros(S.N) if cot_v is None else np.array(cot_v, dtype=np.float64)
    ge = np.zeros((T, S.Ng))
    CS, DS = ha.CS, ha.DS
    for t in range(T - 1, -1, -1):
        qs, ps, Fs, xn, M = tape[t]
        kx, kv = hp.vjp(_t(xn)[None], _t(ps[3])[None], _t(feq), _t([cot_kl[t]]), G)
        lx = lx + kx[0].numpy()
        lv = lv + kv[0].numpy()
        a_ke, a_pe, a_per = cot_hist[t]
        lv = lv + a_ke * ps[3]
        m = (a_pe * S.N / S.L + a_per) * S.dx * M
        nu = -ha._np_K(m, S)
        lx = lx + S.scale * ha._slope(nu, xn, S)
        lq = lx
        lp = lv + CS[3] * S.dt * lq
        for k in (3, 2, 1):
            c = -DS[k] * S.dt * lp
            mu = ha._deposit(c, qs[k - 1], S)
            ge[t] += mu
            nu = -ha._np_K(mu, S)
            lq = lq + c * ha._slope(Fs[k - 1], qs[k - 1], S) + S.scale * ha._slope(nu, qs[k - 1], S)
            lp = lp + CS[k - 1] * S.dt * lq
        lx, lv = lq, lp
    return ge, lx, lv
