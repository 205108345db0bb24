"""Forward mode of the pooled particle features (include/picstep.h: pic_pool_jvp, pic_pool_ln_jvp) restated on the
CPU.  Test infrastructure only.

`jvp`: the contract in float64 NumPy with its operation order written out (every product rounded before its sum, the sums over k
from +0 in ascending order, the integer sums in the contract's units), for the plain layer and -- with gamma and beta -- the
LayerNorm's.  It differs from the device by the libm behind cos, sin and tanh only.  An `audit` dict, if given, collects the
largest |term| / bound of the integer sums and the smallest |argument| a step function saw.
`jvp_ld`: the np.longdouble twin from the float64 q, u, tq and tu on, with plain longdouble sums.
One environment and one direction per call; a tangent that is None is zero.
"""
import functools

import numpy as np

import hp_pool as hp
import hp_pool_ln as hl

LD = np.longdouble
TWO_PI = hp.TWO_PI
JVP_UP = 1.0 + 2.0 ** -40          # the margin of the JVP's bounds
NAMES = ("d_x", "d_v", "d_W", "d_b", "d_gamma", "d_beta")


def _full(t, like):
    return np.zeros_like(np.asarray(like, np.float64)) if t is None else np.asarray(t, np.float64)


def tangent_features(d_x, d_v, L, v_scale):
    """tq, tu in float64 as the contract forms them."""
    return (TWO_PI * np.asarray(d_x, np.float64)) / L, np.asarray(d_v, np.float64) * v_scale


def _dz(W, dW, db, c, s, u, tq, tu, k):
    dz = np.full_like(c, db[k])
    dz = dz + dW[k, 0] * c
    dz = dz + dW[k, 1] * s
    dz = dz + dW[k, 2] * u
    dz = dz + (W[k, 1] * c - W[k, 0] * s) * tq
    dz = dz + W[k, 2] * tu
    return dz


def z_bound(W, dW, db, umax, tqmax, tumax):
    """Z_k [H], the bound of |dz_ik|, as the contract rounds it."""
    Z = np.abs(db)
    Z = Z + np.abs(dW[:, 0])
    Z = Z + np.abs(dW[:, 1])
    Z = Z + np.abs(dW[:, 2]) * umax
    Z = Z + (np.abs(W[:, 0]) + np.abs(W[:, 1])) * tqmax
    Z = Z + np.abs(W[:, 2]) * tumax
    return Z


def bounds(Z, gamma=None, d_gamma=None, d_beta=None, rmax=None):
    """The bound of one term of d_out_k [H]: Z_k (plain) or (|dgamma_k| sqrt(H) + |gamma_k| ((Z_k + (1 + sqrt(H)) Z_max) r_max)) +
    |dbeta_k|, each times 1 + 2^-40."""
    if gamma is None:
        return Z * JVP_UP
    sqrtH = np.sqrt(float(len(Z)))
    bz = (Z + (1.0 + sqrtH) * np.max(Z)) * rmax
    return ((np.abs(d_gamma) * sqrtH + np.abs(gamma) * bz) + np.abs(d_beta)) * JVP_UP


def _dact(z, activation, audit):
    if activation == "tanh":
        h = np.tanh(z)
        return 1.0 - h * h
    hl._note(audit, "n_min", float(np.min(np.abs(z))), smallest=True)
    return np.where(z > 0, 1.0, 0.0)


def _setup(x, v, W, b, L, v_scale, t, gamma, beta):
    ln = gamma is not None
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    q, u = hp.features(x, v, L, v_scale)
    tq, tu = tangent_features(_full(t.get("d_x"), q), _full(t.get("d_v"), q), L, v_scale)
    dW, db = _full(t.get("d_W"), W), _full(t.get("d_b"), b)
    dg, dbe = (_full(t.get("d_gamma"), b), _full(t.get("d_beta"), b)) if ln else (None, None)
    return ln, W, b, q, u, tq, tu, dW, db, dg, dbe


def term_bounds(x, v, W, b, L, activation="tanh", v_scale=1.0, gamma=None, beta=None, eps=1e-5, **t):
    """The contract bound of a term of d_out_k [H] for one environment and direction, from the float64 maxima."""
    ln, W, b, q, u, tq, tu, dW, db, dg, dbe = _setup(x, v, W, b, L, v_scale, t, gamma, beta)
    Z = z_bound(W, dW, db, float(np.max(np.abs(u))), float(np.max(np.abs(tq))), float(np.max(np.abs(tu))))
    if not ln:
        return bounds(Z)
    _, r = hl.stats(np.cos(q), np.sin(q), u, W, b, eps)
    return bounds(Z, np.asarray(gamma, np.float64), dg, dbe, float(np.max(r)))


def jvp(x, v, W, b, L, activation="tanh", v_scale=1.0, gamma=None, beta=None, eps=1e-5, audit=None, **t):
    """d_out [H] of one environment along one direction t = {d_x, d_v [N], d_W [H, 3], d_b, d_gamma, d_beta [H]}."""
    ln, W, b, q, u, tq, tu, dW, db, dg, dbe = _setup(x, v, W, b, L, v_scale, t, gamma, beta)
    c, s = np.cos(q), np.sin(q)
    N, bN, H = len(q), hp.bits_n(len(q)), len(b)
    Z = z_bound(W, dW, db, float(np.max(np.abs(u))), float(np.max(np.abs(tq))), float(np.max(np.abs(tu))))
    out = np.zeros(H)
    if not ln:
        B = bounds(Z)
        for k in range(H):
            a = _dact(hp._pre(W, b, c, s, u, k), activation, audit)
            out[k] = hl._int_sum(a * _dz(W, dW, db, c, s, u, tq, tu, k), B[k], bN, audit, "d_out") / N
        return out
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mu, r = hl.stats(c, s, u, W, b, eps)
    B = bounds(Z, gamma, dg, dbe, float(np.max(r)))
    acc = np.zeros(N)
    for k in range(H):
        acc = acc + _dz(W, dW, db, c, s, u, tq, tu, k)
    dmu = acc / float(H)
    acc = np.zeros(N)
    for k in range(H):
        y = (hp._pre(W, b, c, s, u, k) - mu) * r
        acc = acc + y * (_dz(W, dW, db, c, s, u, tq, tu, k) - dmu)
    p = acc / float(H)
    for k in range(H):
        y, n = hl._norm(c, s, u, W, b, gamma, beta, mu, r, k)
        a = _dact(n, activation, audit)
        e = _dz(W, dW, db, c, s, u, tq, tu, k) - dmu
        dy = (e - y * p) * r
        hl._note(audit, "dy", float(np.max(np.abs(dy))))
        gy, gd = dg[k] * y, gamma[k] * dy
        out[k] = hl._int_sum(a * ((gy + gd) + dbe[k]), B[k], bN, audit, "d_out") / N
    return out


def jvp_ld(x, v, W, b, L, activation="tanh", v_scale=1.0, gamma=None, beta=None, eps=1e-5, **t):
    """d_out [H] in longdouble."""
    ln, W, b, q, u, tq, tu, dW, db, dg, dbe = _setup(x, v, W, b, L, v_scale, t, gamma, beta)
    ql, ul, tql, tul = (a.astype(LD) for a in (q, u, tq, tu))
    c, s = np.cos(ql), np.sin(ql)
    Wl, bl, dWl, dbl = (a.astype(LD) for a in (W, b, dW, db))
    z = bl[None, :] + c[:, None] * Wl[None, :, 0] + s[:, None] * Wl[None, :, 1] + ul[:, None] * Wl[None, :, 2]       # [N, H]
    dz = (dbl[None, :] + c[:, None] * dWl[None, :, 0] + s[:, None] * dWl[None, :, 1] + ul[:, None] * dWl[None, :, 2]
          + (c[:, None] * Wl[None, :, 1] - s[:, None] * Wl[None, :, 0]) * tql[:, None] + tul[:, None] * Wl[None, :, 2])
    act = lambda n: LD(1) - np.tanh(n) ** 2 if activation == "tanh" else np.where(n > 0, LD(1), LD(0))      # noqa: E731
    if not ln:
        return (act(z) * dz).sum(axis=0) / LD(len(c))
    gl, bel, dgl, dbel = (np.asarray(a, np.float64).astype(LD) for a in (gamma, beta, dg, dbe))
    d = z - z.mean(axis=1, keepdims=True)
    r = LD(1) / np.sqrt((d * d).mean(axis=1, keepdims=True) + LD(eps))
    y = d * r
    e = dz - dz.mean(axis=1, keepdims=True)
    dy = (e - y * (y * e).mean(axis=1, keepdims=True)) * r
    dn = dgl[None, :] * y + gl[None, :] * dy + dbel[None, :]
    return (act(gl[None, :] * y + bel[None, :]) * dn).sum(axis=0) / LD(len(c))


def rel_error(got, want, B):
    """max_k |got_k - want_k| / B_k over the units with a bound; a unit without one must be exactly 0."""
    got, B = np.asarray(got), np.asarray(B)
    on = B > 0
    assert np.all(got[~on] == 0.0)
    return float(np.max(np.abs(got[on].astype(LD) - np.asarray(want)[on]) / B[on])) if on.any() else 0.0


# ---- cases ------------------------------------------------------------------------------------------------------------------------
L = hl.L
ACTS = hl.ACTS
FLOOR_SHAPES = hp.FLOOR_SHAPES      # N in {1, 63, 5000, 8193} x H in {1, 5, 64}


def tangents(N, H, seed, ln, lead=(), K=None):
    """Random tangents of every input: d_x, d_v lead + [N]; d_W [H, 3], d_b (d_gamma, d_beta) [H]; a leading K axis if asked."""
    rng = np.random.default_rng(seed)
    k = () if K is None else (K,)
    t = {"d_x": rng.normal(0.0, 1.0, k + lead + (N,)), "d_v": rng.normal(0.0, 1.0, k + lead + (N,)),
         "d_W": rng.normal(0.0, 1.0, k + (H, 3)), "d_b": rng.normal(0.0, 1.0, k + (H,))}
    if ln:
        t["d_gamma"], t["d_beta"] = rng.normal(0.0, 1.0, k + (H,)), rng.normal(0.0, 1.0, k + (H,))
    return t


@functools.lru_cache(maxsize=None)
def floor_case(N, H, ln):
    """(x, v [N], the layer's parameters, the tangents) of one floor shape: box_data's positions, hp_pool_ln's layer."""
    X, V = hp.box_data(1, N, seed=100 * H + N)
    W, b, gamma, beta = hl.layer(H, seed=1)
    kw = dict(gamma=gamma, beta=beta) if ln else {}
    return X[0], V[0], W, b, kw, tangents(N, H, seed=7 * H + N, ln=ln)


@functools.lru_cache(maxsize=None)
def floor():
    """{"plain": ..., "ln": ...}: the largest error of the float64 restatement against its longdouble twin over FLOOR_SHAPES and
    both activations, relative to each output's contract bound; and under "audit" what the terms did there."""
    worst = {"plain": 0.0, "ln": 0.0, "audit": {}}
    for N, H in FLOOR_SHAPES:
        for ln in (False, True):
            x, v, W, b, kw, t = floor_case(N, H, ln)
            for act in ACTS:
                got = jvp(x, v, W, b, L, act, audit=worst["audit"], **kw, **t)
                err = rel_error(got, jvp_ld(x, v, W, b, L, act, **kw, **t), term_bounds(x, v, W, b, L, act, **kw, **t))
                key = "ln" if ln else "plain"
                worst[key] = max(worst[key], err)
    return worst


def bound(ln, N):
    """What a device result may differ from the restatement by, relative to its contract bound: 100 x the floor (the rule of
    DESIGN.md 7c / 7o / 7r) plus 4 N 2^-61 for the integer unit, as hp_pool_ln.bound derives it (the device's maxima may differ
    from NumPy's by an ulp of the libm and so double a unit)."""
    return 100.0 * floor()["ln" if ln else "plain"] + 4.0 * N * 2.0 ** -61


def restated(X, V, W, b, Lb, activation, v_scale=1.0, gamma=None, beta=None, eps=1e-5, **t):
    """The restatement over a batch and K directions, shaped like the device's result [K, E, H]: X, V [E, N]; parameters shared
    or with a leading E; tangents with a leading K (d_x, d_v [K, E, N]; parameters' [K, ...])."""
    E, per_env = len(X), np.ndim(W) == 3
    K = next(len(a) for a in t.values() if a is not None)
    out, Bs = [], []
    for kk in range(K):
        for e in range(E):
            pe = lambda a: None if a is None else (a[e] if per_env else a)      # noqa: E731
            te = {k: None if a is None else (a[kk][e] if (k in ("d_x", "d_v") or per_env) else a[kk]) for k, a in t.items()}
            args = (X[e], V[e], pe(W), pe(b), Lb, activation, v_scale, pe(gamma), pe(beta), eps)
            out.append(jvp(*args, **te))
            Bs.append(term_bounds(*args, **te))
    H = np.shape(b)[-1]
    return np.reshape(out, (K, E, H)), np.reshape(Bs, (K, E, H))


# ---- the grid of the device's parity test (tests/test_gpu_pool_jvp.py): hp_pool_ln's grid with tangents -----------------------------
GRID_N, GRID_H = hl.GRID_N, hl.GRID_H
PARAM_T = {False: ("d_W", "d_b"), True: ("d_W", "d_b", "d_gamma", "d_beta")}


def grid_K(N, H):
    """The directions of a shape of the grid: 8 (full groups only) up to 64 x 1025 and 256 x 63, 3 (a partial group) up to
    256 x 1025 and 64 x 4097, 1 at 256 x 4097 -- the restatement of every direction is what the test's time goes to."""
    return 8 if N * H <= 64 * 1025 else (3 if N * H <= 256 * 1025 else 1)


@functools.lru_cache(maxsize=None)
def grid_tangents(N, H):
    """d_x, d_v [8, 3, N] and two sets of parameter tangents (each name [8, ...]) for hp_pool_ln.grid_case(N, H)."""
    t = tangents(N, H, seed=31 * H + N, ln=True, lead=(3,), K=8)
    t2 = tangents(N, H, seed=37 * H + N, ln=True, K=8)
    pick = lambda d: {k: d[k] for k in PARAM_T[True]}      # noqa: E731
    return t["d_x"], t["d_v"], (pick(t), pick(t2))


@functools.lru_cache(maxsize=None)
def grid_restated(N, H, e, s, act, ln, kk):
    """(d_out [H], its bounds [H]) of environment e of the grid's shape under parameter set s (and that set's tangents) along
    direction kk."""
    X, V, sets, _ = hl.grid_case(N, H)
    dX, dV, tsets = grid_tangents(N, H)
    W, b, gamma, beta = sets[s]
    kw = dict(gamma=gamma, beta=beta) if ln else {}
    t = {k: tsets[s][k][kk] for k in PARAM_T[ln]}
    args = (X[e], V[e], W, b, L, act)
    return jvp(*args, d_x=dX[kk][e], d_v=dV[kk][e], **kw, **t), term_bounds(*args, d_x=dX[kk][e], d_v=dV[kk][e], **kw, **t)


def duality_gap(x, v, W, b, cot, Lb, activation, gamma=None, beta=None, **t):
    """|<cot, jvp> - <vjp, t>| of the two float64 restatements relative to sum_k |cot_k| B_k (B: the JVP's term bounds, which
    bound |d_out_k|), for one environment and direction."""
    ln = gamma is not None
    kw = dict(gamma=gamma, beta=beta) if ln else {}
    lhs = float(np.dot(cot, jvp(x, v, W, b, Lb, activation, **kw, **t)))
    g = hl.vjp(x, v, W, b, gamma, beta, cot, Lb, activation) if ln else hp.vjp(x, v, W, b, cot, Lb, activation)
    rhs = sum(float(np.sum(gi * t[k])) for gi, k in zip(g, NAMES) if t.get(k) is not None)
    return abs(lhs - rhs) / float(np.sum(np.abs(cot) * term_bounds(x, v, W, b, Lb, activation, **kw, **t)))
