"""The pooled particle features with a LayerNorm (include/picstep.h: pic_pool_ln, pic_pool_ln_vjp) restated on the
CPU.  Test infrastructure only.

`forward` / `vjp`: the contract in float64 NumPy with its operation order written out (every product rounded before its sum, the
sums over k from +0 in ascending order, the integer sums in the contract's units).  They differ from the device by the libm
behind cos, sin and tanh only.  An `audit` dict, if given, collects what the CPU tests prove about the terms: the largest
|term| / bound of every integer sum, the largest |y| / sqrt(H) and the smallest |n| a step function saw.
`both_ld`: the np.longdouble twin from the float64 q and u on, with plain longdouble sums.
"""
import functools
import os

import numpy as np

import hp_pool as hp

LD = np.longdouble
TWO_PI = hp.TWO_PI
FWD_UP = 1.0 + 2.0 ** -50          # the margin of the forward's relu bound
VJP_UP = 1.0 + 2.0 ** -40          # ... of the VJP's three bounds


def _note(audit, key, value, smallest=False):
    if audit is not None:
        audit[key] = min(audit.get(key, np.inf), value) if smallest else max(audit.get(key, 0.0), value)


def _int_sum(terms, bound, bN, audit, key):
    """The integer sum of `terms` in the unit of `bound` (+0 for a zero bound), as the device converts it back."""
    if not bound > 0:
        return 0.0
    _note(audit, key, float(np.max(np.abs(terms))) / bound)
    return hp._int_sum(terms, hp._exp(bound) + bN - 61)


def stats(c, s, u, W, b, eps):
    """mu_i and r_i [N]: two walks over k."""
    H = len(b)
    acc = np.zeros_like(c)
    for k in range(H):
        acc = acc + hp._pre(W, b, c, s, u, k)
    mu = acc / float(H)
    acc = np.zeros_like(c)
    for k in range(H):
        d = hp._pre(W, b, c, s, u, k) - mu
        acc = acc + d * d
    return mu, 1.0 / np.sqrt(acc / float(H) + eps)


def _norm(c, s, u, W, b, gamma, beta, mu, r, k):
    y = (hp._pre(W, b, c, s, u, k) - mu) * r
    n = gamma[k] * y
    return y, n + beta[k]


def forward_bound(gamma, beta, activation):
    """B_k of the forward's unit [H] (1 for tanh), as the contract rounds it."""
    if activation == "tanh":
        return np.ones(len(gamma))
    return (np.abs(gamma) * np.sqrt(float(len(gamma))) + np.abs(beta)) * FWD_UP


def forward(x, v, W, b, gamma, beta, period, activation="relu", v_scale=1.0, eps=1e-5, audit=None):
    """out [H] of one environment: x, v [N], W [H, 3], b, gamma, beta [H]."""
    q, u = hp.features(x, v, period, v_scale)
    c, s = np.cos(q), np.sin(q)
    N, bN, H = len(q), hp.bits_n(len(q)), len(b)
    mu, r = stats(c, s, u, W, b, eps)
    B = forward_bound(gamma, beta, activation)
    out = np.zeros(H)
    for k in range(H):
        y, n = _norm(c, s, u, W, b, gamma, beta, mu, r, k)
        _note(audit, "y", float(np.max(np.abs(y))) / np.sqrt(float(H)))
        h = np.tanh(n) if activation == "tanh" else np.where(n > 0, n, 0.0)
        out[k] = _int_sum(h, B[k], bN, audit, "out") / N
    return out


def vjp_bounds(gamma, cot, N, rmax, umax):
    """The bounds of a term of (g_W_k. and g_b_k, g_gamma_k, g_beta_k), [H] each, as the contract rounds them."""
    sqrtH, Nd = np.sqrt(float(len(gamma))), float(N)
    ck, D = np.abs(cot) / Nd, (np.abs(cot) * np.abs(gamma)) / Nd
    bw = (((D + (1.0 + sqrtH) * np.max(D)) * rmax) * (umax if umax > 1.0 else 1.0)) * VJP_UP
    return bw, (ck * sqrtH) * VJP_UP, ck * VJP_UP


def vjp(x, v, W, b, gamma, beta, cot, period, activation="relu", v_scale=1.0, eps=1e-5, audit=None):
    """(g_x [N], g_v [N], g_W [H, 3], g_b, g_gamma, g_beta [H]) of one environment for a cotangent cot [H]."""
    q, u = hp.features(x, v, period, v_scale)
    c, s = np.cos(q), np.sin(q)
    N, bN, H = len(q), hp.bits_n(len(q)), len(b)
    Nd, Hd = float(N), float(H)
    mu, r = stats(c, s, u, W, b, eps)
    bw, bg, bb = vjp_bounds(gamma, cot, N, float(np.max(r)), float(np.max(np.abs(u))))
    gW, gb, gg, gbe = np.zeros((H, 3)), np.zeros(H), np.zeros(H), np.zeros(H)

    def dn_of(n, k):
        if activation == "tanh":
            h = np.tanh(n)
            a = 1.0 - h * h
        else:
            _note(audit, "n_min", float(np.min(np.abs(n))), smallest=True)
            a = np.where(n > 0, 1.0, 0.0)
        return (cot[k] * a) / Nd

    m1, m2 = np.zeros(N), np.zeros(N)
    for k in range(H):
        y, n = _norm(c, s, u, W, b, gamma, beta, mu, r, k)
        dn = dn_of(n, k)
        dy = dn * gamma[k]
        m1 = m1 + dy
        m2 = m2 + dy * y
        gg[k] = _int_sum(dn * y, bg[k], bN, audit, "g_gamma")
        gbe[k] = _int_sum(dn, bb[k], bN, audit, "g_beta")
    m1, m2 = m1 / Hd, m2 / Hd
    sx, sv = np.zeros(N), np.zeros(N)
    for k in range(H):
        y, n = _norm(c, s, u, W, b, gamma, beta, mu, r, k)
        dy = dn_of(n, k) * gamma[k]
        dz = ((dy - m1) - y * m2) * r
        sx = sx + dz * (W[k, 1] * c - W[k, 0] * s)
        sv = sv + dz * W[k, 2]
        gW[k] = [_int_sum(dz * c, bw[k], bN, audit, "g_W"), _int_sum(dz * s, bw[k], bN, audit, "g_W"),
                 _int_sum(dz * u, bw[k], bN, audit, "g_W")]
        gb[k] = _int_sum(dz, bw[k], bN, audit, "g_b")
    return (TWO_PI / period) * sx, v_scale * sv, gW, gb, gg, gbe


# ---- the extended-precision twin -----------------------------------------------------------------------------------------------
def both_ld(x, v, W, b, gamma, beta, cot, period, activation="relu", v_scale=1.0, eps=1e-5):
    """(out, g_x, g_v, g_W, g_b, g_gamma, g_beta) in longdouble (the gradients None without a cotangent)."""
    q, u = hp.features(x, v, period, v_scale)
    ql, ul = q.astype(LD), u.astype(LD)
    c, s = np.cos(ql), np.sin(ql)
    Wl, bl, gl, bel = (np.asarray(a, np.float64).astype(LD) for a in (W, b, gamma, beta))
    N = LD(len(c))
    z = bl[None, :] + c[:, None] * Wl[None, :, 0] + s[:, None] * Wl[None, :, 1] + ul[:, None] * Wl[None, :, 2]      # [N, H]
    d = z - z.mean(axis=1, keepdims=True)
    r = LD(1) / np.sqrt((d * d).mean(axis=1, keepdims=True) + LD(eps))
    y = d * r
    n = gl[None, :] * y + bel[None, :]
    if activation == "tanh":
        h = np.tanh(n)
        a = LD(1) - h * h
    else:
        h = np.where(n > 0, n, LD(0))
        a = np.where(n > 0, LD(1), LD(0))
    out = h.sum(axis=0) / N
    if cot is None:
        return (out,) + (None,) * 6
    dn = np.asarray(cot, np.float64).astype(LD)[None, :] * a / N
    dy = dn * gl[None, :]
    dz = (dy - dy.mean(axis=1, keepdims=True) - y * (dy * y).mean(axis=1, keepdims=True)) * r
    gx = (LD(TWO_PI) / LD(period)) * ((dz @ Wl[:, 1]) * c - (dz @ Wl[:, 0]) * s)
    gv = LD(v_scale) * (dz @ Wl[:, 2])
    return out, gx, gv, np.stack([c @ dz, s @ dz, ul @ dz], axis=1), dz.sum(axis=0), (dn * y).sum(axis=0), dn.sum(axis=0)


# ---- scales the errors are measured against: each output's contract bound --------------------------------------------------------
def forward_scale(gamma, beta, activation):
    """max(1, B_k) [H]."""
    return np.maximum(1.0, forward_bound(gamma, beta, activation))


def vjp_scales(x, v, W, b, gamma, cot, period, v_scale, eps):
    """Bounds of |g_x_i|, |g_v_i| (scalars) and of the six parameter sums (N terms of their bound: g_W / g_b, g_gamma, g_beta,
    [H] each), from the float64 r_max and u_max of the environment."""
    q, u = hp.features(x, v, period, v_scale)
    _, r = stats(np.cos(q), np.sin(q), u, W, b, eps)
    umax = float(np.max(np.abs(u)))
    bw, bg, bb = vjp_bounds(gamma, cot, len(q), float(np.max(r)), umax)
    bz = bw / max(1.0, umax)                                         # the bound of |dz_ik|
    sx = (TWO_PI / period) * float(np.sum(bz * (np.abs(W[:, 0]) + np.abs(W[:, 1]))))
    sv = abs(v_scale) * float(np.sum(bz * np.abs(W[:, 2])))
    N = len(q)
    return sx, sv, N * bw, N * bg, N * bb


def errors(got_out, got_vjp, ref, x, v, W, b, gamma, beta, cot, period, activation, v_scale=1.0, eps=1e-5):
    """(forward error, VJP error) of one environment's results against `ref` (both_ld's tuple, or the restatement's (out,
    *vjp)), each relative to its contract bound.  got_vjp = (g_x, g_v, g_W, g_b, g_gamma, g_beta), entries may be None."""
    ef = eg = 0.0
    if got_out is not None:
        ef = float(np.max(np.abs(np.asarray(got_out).astype(LD) - ref[0]) / forward_scale(gamma, beta, activation)))
    if got_vjp is not None:
        sx, sv, sw, sg, sb = vjp_scales(x, v, W, b, gamma, cot, period, v_scale, eps)
        for got, want, scale in zip(got_vjp, ref[1:], (sx, sv, sw[:, None], sw, sg, sb)):
            if got is not None:
                eg = max(eg, float(np.max(np.abs(np.asarray(got).astype(LD) - want) / scale)))
    return ef, eg


# ---- the grid of the device's parity test (tests/test_gpu_pool_ln.py) and the floor over it --------------------------------------
L = 50.0
GRID_N = (1, 2, 63, 1025, 4097)
GRID_H = (1, 2, 5, 64, 256)
ACTS = ("relu", "tanh")
N_MIN = 1e-9                    # no |n| that a relu step function sees may be nearer to the kink: no ulp of a libm can flip it


def layer(H, seed, lead=()):
    """(W, b, gamma, beta) of a policy's size; gamma and beta away from LayerNorm's defaults 1 / 0."""
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 0.5, lead + (H, 3)), rng.normal(0.0, 0.1, lead + (H,)), rng.uniform(-1.5, 1.5, lead + (H,)),
            rng.uniform(-1.0, 1.0, lead + (H,)))


@functools.lru_cache(maxsize=None)
def grid_case(N, H):
    """The data of one shape of the grid: X, V [3, N] (box_data: the box's edges among the positions), two parameter sets and
    cot [3, H]."""
    X, V = hp.box_data(3, N, seed=100 * H + N)
    return X, V, (layer(H, seed=1), layer(H, seed=2)), np.random.default_rng(H).normal(0.0, 1.0, (3, H))


@functools.lru_cache(maxsize=None)
def restated(N, H, e, s, activation):
    """(out, g_x, g_v, g_W, g_b, g_gamma, g_beta) of environment e of the grid's shape under parameter set s, and its audit."""
    X, V, sets, cot = grid_case(N, H)
    audit = {}
    out = forward(X[e], V[e], *sets[s], L, activation, audit=audit)
    return (out,) + vjp(X[e], V[e], *sets[s], cot[e], L, activation, audit=audit), audit


@functools.lru_cache(maxsize=None)
def floor():
    """{"forward": ..., "vjp": ...}: the largest error of the float64 restatement against its longdouble twin over the grid (its
    environment 0 under its first parameter set, both activations), relative to each output's contract bound."""
    worst = {"forward": 0.0, "vjp": 0.0}
    for N in GRID_N:
        for H in GRID_H:
            X, V, sets, cot = grid_case(N, H)
            for act in ACTS:
                got = restated(N, H, 0, 0, act)[0]
                ref = both_ld(X[0], V[0], *sets[0], cot[0], L, act)
                ef, eg = errors(got[0], got[1:], ref, X[0], V[0], *sets[0], cot[0], L, act)
                worst["forward"], worst["vjp"] = max(worst["forward"], ef), max(worst["vjp"], eg)
    return worst


def bound(kind, N):
    """What a device result may differ from the restatement by, relative to its contract bound: 100 x the floor (the rule of
    DESIGN.md 7c / 7o / 7r) plus the resolution of the integer unit.  Each of the two sums is within N half units of its exact
    value, a unit is 2^(e + bits_n - 61) <= 2 N 2^-61 2^e, and 2^e is at most twice the bound: 2 N 2^-61 of the scale as in 7r,
    twice that because r_max and u_max of the device may differ from NumPy's by an ulp of the libm, which can move a bound across
    a power of two and so double the device's unit."""
    return 100.0 * floor()[kind] + 4.0 * N * 2.0 ** -61


# ---- the reference encoder's recorded results (tests/golden/make_golden_g19.py) ------------------------------------------------------
G19 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_particle_encoder.npz"))
PHI = ("phi.0.weight", "phi.0.bias", "phi.1.weight", "phi.1.bias")
G19_CASES = tuple(str(c) for c in G19["cases"])


def g19_case(pre):
    """(the case's arrays without their prefix, its state dict, period = L_ref x_norm, v_scale = 1 / v_norm)."""
    g = {k[len(pre) + 1:]: G19[k] for k in G19.files if k.startswith(pre + "_")}
    sd = {k[3:]: v for k, v in g.items() if k.startswith("sd_")}
    return g, sd, float(G19["L"]) * float(g["x_norm"]), 1.0 / float(g["v_norm"])


@functools.lru_cache(maxsize=None)
def g19_restated(pre):
    """(out [E, H], the six gradients per environment) of the restatement on a g19 case, for its cot_phi."""
    g, sd, period, v_scale = g19_case(pre)
    p = [sd[k] for k in PHI]
    outs, grads = [], []
    for e in range(len(g["x"])):
        outs.append(forward(g["x"][e], g["v"][e], *p, period, "relu", v_scale))
        grads.append(vjp(g["x"][e], g["v"][e], *p, g["cot_phi"][e], period, "relu", v_scale))
    return np.stack(outs), grads


def g19_errors(pre, out, grads, cot=None, want=None):
    """(forward error, VJP error) of results on a g19 case against its recorded ones, relative to each output's contract bound:
    out [E, H] against phi_mean; grads = (g_x [E, N], g_v, g_W, g_b, g_gamma, g_beta), the parameters' summed over the
    environments as torch sums them, against gphi_* -- or against `want` for another cotangent `cot` [E, H]."""
    g, sd, period, v_scale = g19_case(pre)
    p = [sd[k] for k in PHI]
    cot = g["cot_phi"] if cot is None else cot
    want = [g["gphi_" + k] for k in ("x", "v") + PHI] if want is None else want
    E = len(g["x"])
    ef = eg = 0.0
    if out is not None:
        ef = float(np.max(np.abs(out - g["phi_mean"]) / forward_scale(p[2], p[3], "relu")))
    scales = [vjp_scales(g["x"][e], g["v"][e], p[0], p[1], p[2], cot[e], period, v_scale, 1e-5) for e in range(E)]
    for e in range(E):
        eg = max(eg, float(np.max(np.abs(grads[0][e] - want[0][e])) / scales[e][0]),
                 float(np.max(np.abs(grads[1][e] - want[1][e])) / scales[e][1]))
    for i, j in enumerate((2, 2, 3, 4)):
        scale = sum(s[j] for s in scales)
        eg = max(eg, float(np.max(np.abs(grads[2 + i] - want[2 + i]) / (scale[:, None] if i == 0 else scale))))
    return ef, eg


@functools.lru_cache(maxsize=None)
def g19_restatement_error():
    """The largest g19_errors of the restatement itself over the cases."""
    ef = eg = 0.0
    for pre in G19_CASES:
        out, grads = g19_restated(pre)
        E = len(out)
        summed = [np.stack([gr[i] for gr in grads]) for i in (0, 1)] + [sum(grads[e][i] for e in range(E)) for i in (2, 3, 4, 5)]
        a, c = g19_errors(pre, out, summed)
        ef, eg = max(ef, a), max(eg, c)
    return ef, eg
