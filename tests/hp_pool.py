"""The pooled particle features (include/picstep.h: pic_pool, pic_pool_vjp) restated on the CPU.  Test
infrastructure only.

`forward` / `vjp`: the contract in float64 NumPy with its operation order written out (every product rounded before its sum, the
integer sums in the contract's units).  They differ from the device by the libm behind cos, sin and tanh only.
`forward_ld` / `vjp_ld`: the np.longdouble twin.  It takes the float64 q and u (the contract's inputs of the trigonometry and of
the layer) and is extended from there, with plain longdouble sums.
"""
import functools

import numpy as np

TWO_PI = 2.0 * np.pi
ROUND_UP = 1.0 + 2.0 ** -50
LD = np.longdouble


def bits_n(N):
    b = 0
    while (1 << b) < N:
        b += 1
    return b


def _exp(bound):
    """e with 2^e > bound (ilogb + 1), for a finite positive double."""
    return int(np.frexp(bound)[1])


def features(x, v, L, v_scale):
    """q, u in float64 as the contract forms them."""
    q = (TWO_PI * np.asarray(x, np.float64)) / L
    u = np.asarray(v, np.float64) * v_scale
    return q, u


def forward_bound(W, b, u, activation):
    """B_k of the forward's unit [H] (1 for tanh), as the contract rounds it."""
    if activation == "tanh":
        return np.ones(len(b))
    umax = np.max(np.abs(u))
    return (((np.abs(W[:, 0]) + np.abs(W[:, 1])) + np.abs(W[:, 2]) * umax) + np.abs(b)) * ROUND_UP


def forward_exp(W, b, u, activation):
    """e_k [H] with 2^e_k >= B_k: the unit is 2^(e_k + bits_n(N) - 61).  None where B_k = 0."""
    if activation == "tanh":
        return [0] * len(b)
    return [_exp(B) if B > 0 else None for B in forward_bound(W, b, u, activation)]


def _int_sum(terms, ue):
    """sum of round-to-nearest-even(terms / 2^ue) as an exact integer, back in float64 as the device converts it."""
    r = np.rint(np.ldexp(terms, -ue))
    assert np.all(np.abs(r) <= 2.0 ** 61)                    # (so the int64 sum of N <= 2^b of them is exact)
    return float(np.ldexp(np.float64(int(r.astype(np.int64).sum())), ue))


def _pre(W, b, c, s, u, k):
    z = np.full_like(c, b[k])
    z = z + W[k, 0] * c
    z = z + W[k, 1] * s
    z = z + W[k, 2] * u
    return z


def _act(z, activation):
    return np.tanh(z) if activation == "tanh" else np.where(z > 0, z, 0.0)


def forward(x, v, W, b, L, activation="tanh", v_scale=1.0):
    """out [H] of one environment: x, v [N], W [H, 3], b [H]."""
    q, u = features(x, v, L, v_scale)
    c, s = np.cos(q), np.sin(q)
    N, bN = len(q), bits_n(len(q))
    es = forward_exp(W, b, u, activation)
    out = np.zeros(len(b))
    for k in range(len(b)):
        if es[k] is None:
            continue
        out[k] = _int_sum(_act(_pre(W, b, c, s, u, k), activation), es[k] + bN - 61) / N
    return out


def vjp_bound(cot, u, N):
    """The bound of the parameter sums' terms [H]: (|cot_k| / N) max(1, u_max)."""
    umax = np.max(np.abs(u))
    return (np.abs(cot) / float(N)) * (umax if umax > 1.0 else 1.0)


def vjp(x, v, W, b, cot, L, activation="tanh", v_scale=1.0):
    """(g_x [N], g_v [N], g_W [H, 3], g_b [H]) of one environment for a cotangent cot [H]."""
    q, u = features(x, v, L, v_scale)
    c, s = np.cos(q), np.sin(q)
    N, bN, H = len(q), bits_n(len(q)), len(b)
    bound = vjp_bound(cot, u, N)
    sx, sv = np.zeros(N), np.zeros(N)
    gW, gb = np.zeros((H, 3)), np.zeros(H)
    for k in range(H):
        z = _pre(W, b, c, s, u, k)
        if activation == "tanh":
            h = np.tanh(z)
            a = 1.0 - h * h
        else:
            a = np.where(z > 0, 1.0, 0.0)
        r = (cot[k] * a) / float(N)
        sx = sx + r * (W[k, 1] * c - W[k, 0] * s)
        sv = sv + r * W[k, 2]
        if bound[k] > 0:
            ue = _exp(bound[k]) + bN - 61
            gW[k] = [_int_sum(r * c, ue), _int_sum(r * s, ue), _int_sum(r * u, ue)]
            gb[k] = _int_sum(r, ue)
    return (TWO_PI / L) * sx, v_scale * sv, gW, gb


# ---- the extended-precision twin -----------------------------------------------------------------------------------------------
def _ld_parts(x, v, W, b, L, v_scale):
    q, u = features(x, v, L, v_scale)
    ql, ul = q.astype(LD), u.astype(LD)
    c, s = np.cos(ql), np.sin(ql)
    Wl, bl = np.asarray(W, np.float64).astype(LD), np.asarray(b, np.float64).astype(LD)
    z = bl[None, :] + c[:, None] * Wl[None, :, 0] + s[:, None] * Wl[None, :, 1] + ul[:, None] * Wl[None, :, 2]      # [N, H]
    return c, s, ul, Wl, z


def both_ld(x, v, W, b, cot, L, activation="tanh", v_scale=1.0):
    """(out, g_x, g_v, g_W, g_b) in longdouble, the activations computed once."""
    c, s, u, Wl, z = _ld_parts(x, v, W, b, L, v_scale)
    if activation == "tanh":
        h = np.tanh(z)
        a = LD(1) - h * h
    else:
        h = np.where(z > 0, z, LD(0))
        a = np.where(z > 0, LD(1), LD(0))
    out = h.sum(axis=0) / LD(len(c))
    if cot is None:
        return out, None, None, None, None
    r = np.asarray(cot, np.float64).astype(LD)[None, :] * a / LD(len(c))                                             # [N, H]
    gx = (LD(TWO_PI) / LD(L)) * ((r @ Wl[:, 1]) * c - (r @ Wl[:, 0]) * s)
    gv = LD(v_scale) * (r @ Wl[:, 2])
    gW = np.stack([c @ r, s @ r, u @ r], axis=1)
    return out, gx, gv, gW, r.sum(axis=0)


def forward_ld(x, v, W, b, L, activation="tanh", v_scale=1.0):
    return both_ld(x, v, W, b, None, L, activation, v_scale)[0]


def vjp_ld(x, v, W, b, cot, L, activation="tanh", v_scale=1.0):
    return both_ld(x, v, W, b, cot, L, activation, v_scale)[1:]


# ---- scales the errors are measured against ---------------------------------------------------------------------------------------
def forward_scale(W, b, u, activation):
    """max(1, B_k) [H]."""
    return np.maximum(1.0, forward_bound(W, b, u, activation))


def vjp_scales(W, cot, u, N, L, v_scale):
    """Bounds of |g_x_i|, |g_v_i| (scalars) and of |g_W_k.|, |g_b_k| ([H]; N terms of the parameter bound each)."""
    rb = np.abs(cot) / float(N)
    sx = (TWO_PI / L) * float(np.sum(rb * (np.abs(W[:, 0]) + np.abs(W[:, 1]))))
    sv = abs(v_scale) * float(np.sum(rb * np.abs(W[:, 2])))
    return sx, sv, N * vjp_bound(cot, u, N)


def case(N, H, seed, L=50.0):
    """A reproducible environment: positions over a few box lengths, velocities of a bump-on-tail's size, a policy-sized layer."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5 * L, 2.5 * L, N)
    v = rng.normal(0.0, 2.0, N)
    W = rng.normal(0.0, 0.5, (H, 3))
    b = rng.normal(0.0, 0.1, H)
    cot = rng.normal(0.0, 1.0, H)
    return x, v, W, b, cot


# ---- the floor: float64 restatement against its longdouble twin ------------------------------------------------------------------
FLOOR_SHAPES = [(N, H) for N in (1, 63, 5000, 8193) for H in (1, 5, 64)]


def errors(got_out, got_vjp, x, v, W, b, cot, L, activation, v_scale=1.0):
    """(forward error, VJP error) of one environment's results against the longdouble twin, each relative to its scale:
    max(1, B_k) for out_k, the bounds of vjp_scales for the gradients.  got_vjp = (g_x, g_v, g_W, g_b), entries may be None."""
    q, u = features(x, v, L, v_scale)
    ef = eg = 0.0
    if got_out is not None:
        ref = forward_ld(x, v, W, b, L, activation, v_scale)
        ef = float(np.max(np.abs(np.asarray(got_out).astype(LD) - ref) / forward_scale(W, b, u, activation)))
    if got_vjp is not None:
        ref = vjp_ld(x, v, W, b, cot, L, activation, v_scale)
        sx, sv, sp = vjp_scales(W, cot, u, len(q), L, v_scale)
        for got, want, scale in zip(got_vjp, ref, (sx, sv, sp[:, None], sp)):
            if got is not None:
                eg = max(eg, float(np.max(np.abs(np.asarray(got).astype(LD) - want) / scale)))
    return ef, eg


@functools.lru_cache(maxsize=None)
def floor():
    """{"forward": ..., "vjp": ...}: the largest error of the float64 restatement against its longdouble twin over FLOOR_SHAPES and
    both activations.  It holds the rounding of the float64 arithmetic and of the integer units."""
    worst = {"forward": 0.0, "vjp": 0.0}
    for N, H in FLOOR_SHAPES:
        for activation in ("tanh", "relu"):
            x, v, W, b, cot = case(N, H, seed=1000 * H + N)
            ef, eg = errors(forward(x, v, W, b, 50.0, activation), vjp(x, v, W, b, cot, 50.0, activation), x, v, W, b, cot, 50.0,
                            activation)
            worst["forward"], worst["vjp"] = max(worst["forward"], ef), max(worst["vjp"], eg)
    return worst


def bound(kind, N):
    """What a device result may differ from the longdouble twin by, relative to its scale: 100 x the floor (the rule of DESIGN.md
    7c / 7o) plus the resolution of the integer unit, N 2^-61 of the unit's bound 2^(e_k) -- which is at most twice the scale."""
    return 100.0 * floor()[kind] + 2.0 * N * 2.0 ** -61


def fd_error(fwd, grad, x, v, W, b, cot, eps, seed):
    """|<g, d> - central difference of <cot, out>| / |<g, d>| along one random direction d in (x, v, W, b); fwd(x, v, W, b) ->
    out [H], grad(x, v, W, b) -> (g_x, g_v, g_W, g_b)."""
    rng = np.random.default_rng(seed)
    d = [rng.standard_normal(a.shape) for a in (x, v, W, b)]
    g = grad(x, v, W, b)
    lin = sum(float(np.sum(np.asarray(gi) * di)) for gi, di in zip(g, d))
    f = lambda sgn: float(np.dot(cot, fwd(*(a + sgn * eps * di for a, di in zip((x, v, W, b), d)))))
    return abs(lin - (f(1.0) - f(-1.0)) / (2.0 * eps)) / abs(lin)


# ---- the passes' launch plan (csrc/host_blocks.h: pool_plan), mirrored; tests/test_pool_cpu.py pins it against the C++ ---------
CHUNK_TILES = 512               # tiles of 2 particles in a workgroup's chunk


def plan(E, N):
    """{"nchunks", "wpe", "chunks_per_wg", "workgroups"} of a pool call on E environments of N particles."""
    nchunks = -(-((N + 1) // 2) // CHUNK_TILES)
    wpe = max(1, min(-(-4096 // E), nchunks))
    cpw = -(-nchunks // wpe)
    return {"nchunks": nchunks, "wpe": wpe, "chunks_per_wg": cpw, "workgroups": -(-nchunks // cpw)}


# ---- data and cases of the edge tests (tests/test_gpu_pool_edges.py and their CPU companions) ------------------------------------
def box_data(E, N, seed, L=50.0):
    """Wrapped positions with the box's edges among them (-0.0, the last double below L), velocities of a bump-on-tail's size."""
    rng = np.random.default_rng(seed)
    X, V = rng.uniform(0.0, L, (E, N)), rng.normal(0.0, 2.0, (E, N))
    X[:, 0] = -0.0
    if N >= 3:
        X[:, 1] = np.nextafter(L, 0.0)
    return X, V


def layer(H, seed, lead=()):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.5, lead + (H, 3)), rng.normal(0.0, 0.1, lead + (H,))


# v_scale and L: the exact powers of two (and -2), and the parity matrix
V_SCALES_EXACT = (2.0 ** -20, 2.0 ** 7, -2.0)
V_SCALES = (0.37, -3.0, 1e3)
BOX_LENGTHS = (TWO_PI, 0.1, 1000.0)
SCALE_NS, SCALE_H = (2, 1025), 5
# every (L, v_scale, N, H) a device test compares with the twin under bound(): the restatement alone must be inside it there
BOUND_SETS = sorted({(Lb, s, N, SCALE_H) for Lb in BOX_LENGTHS for s in V_SCALES for N in SCALE_NS}
                    | {(50.0, s, 1025, SCALE_H) for s in V_SCALES_EXACT + (1.0,)}
                    | {(Lb, s, N, SCALE_H) for Lb in (50.0,) + BOX_LENGTHS for s in (1.0, 2.0 ** -20) for N in SCALE_NS})


def scale_case(Lb, s, N, H):
    """One environment of the v_scale / L tests: (X [2, N], V, W, b, cot [2, H])."""
    X, V = box_data(2, N, seed=N + H, L=Lb)
    W, b = layer(H, seed=3)
    return X, V, W, b, np.random.default_rng(H).normal(0.0, 1.0, (2, H))


def batch_errors(out, g, X, V, W, b, cot, L, activation, v_scale=1.0, skip=()):
    """(forward error, VJP error): the worst of errors() over the environments of a batch.  out [E, H] or None; g: pool_vjp's
    dict or None (entries may be None); W [E, H, 3] and b [E, H] for per-environment parameters -- shared ones have one summed
    gradient, which is not looked at here.  The hidden units in `skip` are left out of the forward's comparison."""
    ef = eg = 0.0
    keep = [k for k in range(np.shape(b)[-1]) if k not in skip]
    for e in range(len(X)):
        per_env = np.ndim(W) == 3
        We, be = (W[e], b[e]) if per_env else (W, b)
        gv = None
        if g is not None:
            pick = lambda k: None if g[k] is None else np.asarray(g[k])[e]
            gv = (pick("g_x"), pick("g_v"), pick("g_W") if per_env else None, pick("g_b") if per_env else None)
        if out is not None and skip:
            q, u = features(X[e], V[e], L, v_scale)
            ref = forward_ld(X[e], V[e], We, be, L, activation, v_scale)
            d = np.abs(np.asarray(out)[e].astype(LD) - ref) / forward_scale(We, be, u, activation)
            ef = max(ef, float(np.max(d[keep])))
            a, c = errors(None, gv, X[e], V[e], We, be, cot[e], L, activation, v_scale) if gv else (0.0, 0.0)
        else:
            a, c = errors(None if out is None else np.asarray(out)[e], gv, X[e], V[e], We, be,
                          None if cot is None else cot[e], L, activation, v_scale)
        ef, eg = max(ef, a), max(eg, c)
    return ef, eg


def restated(X, V, W, b, cot, L, activation, v_scale=1.0, vjp_too=True):
    """The float64 restatement over a batch, shaped like the device's results: out [E, H] and pool_vjp's dict (per-environment
    gradients when W is [E, H, 3], else the environments' sum in ascending order)."""
    per_env = np.ndim(W) == 3
    pe = lambda e: (W[e], b[e]) if per_env else (W, b)
    out = np.stack([forward(X[e], V[e], *pe(e), L, activation, v_scale) for e in range(len(X))])
    if not vjp_too:
        return out, None
    gs = [vjp(X[e], V[e], *pe(e), cot[e], L, activation, v_scale) for e in range(len(X))]
    g = {"g_x": np.stack([a[0] for a in gs]), "g_v": np.stack([a[1] for a in gs])}
    if per_env:
        g["g_W"], g["g_b"] = np.stack([a[2] for a in gs]), np.stack([a[3] for a in gs])
    else:
        g["g_W"], g["g_b"] = gs[0][2], gs[0][3]
        for a in gs[1:]:
            g["g_W"], g["g_b"] = g["g_W"] + a[2], g["g_b"] + a[3]
    return out, g


# activation edges: N = 1000, H = 6, E = 2
EDGE_N, EDGE_H, EDGE_E = 1000, 6, 2


def edge_layer():
    """W [6, 3], b [6]: row 0 = (0, 0, 1), -1 (relu's kink at u = 1), row 1 with W_12 = 40 (tanh saturates for |u| > 1), row 2
    all zero (B_2 = 0), rows 3..5 a policy's size."""
    W, b = layer(EDGE_H, seed=17)
    W[0], b[0] = (0.0, 0.0, 1.0), -1.0
    W[1, 2] = 40.0
    W[2], b[2] = 0.0, 0.0
    return W, b


def edge_cot():
    return np.random.default_rng(18).normal(0.0, 1.0, (EDGE_E, EDGE_H))


def kink_velocities(scale):
    """(V [2, 1000], v_scale) with u = V v_scale = 1.0 exactly at the even particles; the odd ones have u < 1 in environment 0
    and u = 3 in environment 1.  scale = 1: v = 1, v_scale = 1; scale = 2: v = 2, v_scale = 0.5 (the same u, bit for bit)."""
    V = np.ones((EDGE_E, EDGE_N))
    V[0, 1::2] = np.random.default_rng(19).uniform(-3.0, 0.99, EDGE_N // 2)
    V[1, 1::2] = 3.0
    return V * scale, 1.0 / scale


def saturating_velocities():
    """V [2, 1000]: |v| in [1.5, 4] with random signs in environment 0 (every particle saturates row 1), a bump-on-tail's size in
    environment 1."""
    rng = np.random.default_rng(20)
    V = rng.normal(0.0, 2.0, (EDGE_E, EDGE_N))
    V[0] = rng.uniform(1.5, 4.0, EDGE_N) * rng.choice([-1.0, 1.0], EDGE_N)
    return V
