"""The pooled particle features (pic_pool, pic_pool_vjp, control/pool.py) where tests/test_gpu_pool.py does not go:
workgroups that walk more than one chunk, v_scale and L other than 1 and 50, N and H at the chunk's and the layer's limits, the
activations' edges, the NaN rule row by row, switched-off outputs and the torch op's routing, and one handle through calls of
changing shape.  Every device result is compared with the longdouble twin of tests/hp_pool.py under hp.bound, or with another
device result bit for bit; tests/test_pool_cpu.py shows the restatement alone inside that bound at every parameter set used here.

What the contract leaves open is not asserted: g_x, g_v and the other parameter rows of an environment with a non-finite
parameter row or cotangent, and the VJP where relu's B_k overflows."""
import itertools

import numpy as np
import pytest
import torch

import hp_pool as hp
from conftest import record_measure
from test_gpu_pool import ACTS, L, _cuda, _data, _env, _env_errors, _layer, _np, _param_error, _same, _same_results

pytestmark = pytest.mark.gpu

KEYS = ("g_x", "g_v", "g_W", "g_b")


def _env_L(E, N, Lb):
    from ocplasma_amd.env.batched import BatchedPIC
    return BatchedPIC(E, N, 64, L=Lb, dt=0.1)


def _per_env(W, b, E):
    return np.broadcast_to(W, (E,) + W.shape).copy(), np.broadcast_to(b, (E,) + b.shape).copy()


def _measure(name, worst, ef=0.0, eg=0.0):
    worst["forward"], worst["vjp"] = max(worst["forward"], ef), max(worst["vjp"], eg)
    record_measure(f"pool_edges_{name}_forward", worst["forward"])
    record_measure(f"pool_edges_{name}_vjp", worst["vjp"])


def _pos_zero(a):
    a = _np(a)
    return bool(np.all(a == 0) and not np.signbit(a).any())


# ---- 1. workgroups of more than one chunk --------------------------------------------------------------------------------------------
MULTI_CHUNK = [(4096, 1025),        # the second chunk holds one tile with one particle
               (4096, 2561),        # three chunks, the last partial and odd
               (1366, 3075)]        # two workgroups of two chunks, the second partial
MULTI_H = 5


def _three_rows(N):
    X3, V3 = hp.box_data(3, N, seed=N)
    W, b = hp.layer(MULTI_H, seed=1)
    return X3, V3, W, b, np.random.default_rng(N + 1).normal(0.0, 1.0, (3, MULTI_H))


@pytest.mark.parametrize("E,N", MULTI_CHUNK)
def test_multi_chunk_workgroups_give_the_one_chunk_bits(E, N):
    """A batch of row[e % 3], per-environment parameters: every environment with the same row has the same bits, environments
    0, 1, 2 those of a one-environment handle (one chunk per workgroup), and these are within the bound of the twin."""
    assert hp.plan(E, N)["chunks_per_wg"] >= 2 and hp.plan(1, N)["chunks_per_wg"] == 1
    X3, V3, W, b, cot3 = _three_rows(N)
    idx = torch.arange(E, device="cuda") % 3
    tX, tV, tc = (t[idx].contiguous() for t in _cuda(X3, V3, cot3))
    tW, tb = (t.expand((E,) + t.shape).contiguous() for t in _cuda(W, b))
    big, one = _env(E, N), _env(1, N)
    worst = {"forward": 0.0, "vjp": 0.0}
    for act in ACTS:
        out, g = big.pool(tW, tb, act, x=tX, v=tV), big.pool_vjp(tW, tb, tc, act, x=tX, v=tV)
        for name, a in [("out", out)] + [(k, g[k]) for k in KEYS]:
            bits = a.view(torch.int64)
            assert torch.equal(bits, bits[:3][idx]), (act, name)
        for r in range(3):
            o1 = one.pool(W[None], b[None], act, x=X3[r:r + 1], v=V3[r:r + 1])
            g1 = one.pool_vjp(W[None], b[None], cot3[r:r + 1], act, x=X3[r:r + 1], v=V3[r:r + 1])
            assert _same(o1[0], out[r]) and all(_same(g1[k][0], g[k][r]) for k in KEYS), (act, r)
            ef, eg = hp.errors(o1[0], tuple(g1[k][0] for k in KEYS), X3[r], V3[r], W, b, cot3[r], L, act)
            _measure(f"multi_chunk_{E}x{N}", worst, ef, eg)
    assert worst["forward"] < hp.bound("forward", N) and worst["vjp"] < hp.bound("vjp", N), worst
    big.close()
    one.close()


def test_multi_chunk_shared_parameter_gradient():
    """Shared parameters at 4096 x 1025: the gradient is the sum over the environments, that is the three rows' references
    weighted with how often each row occurs, relative to the sum of the environments' scales."""
    E, N = MULTI_CHUNK[0]
    assert hp.plan(E, N)["chunks_per_wg"] >= 2
    X3, V3, W, b, cot3 = _three_rows(N)
    idx = torch.arange(E, device="cuda") % 3
    tX, tV, tc = (t[idx].contiguous() for t in _cuda(X3, V3, cot3))
    count = [len(range(r, E, 3)) for r in range(3)]
    env = _env(E, N)
    worst = 0.0
    for act in ACTS:
        g = env.pool_vjp(W, b, tc, act, x=tX, v=tV)
        refs, scales = [], []
        for r in range(3):
            ref = hp.both_ld(X3[r], V3[r], W, b, cot3[r], L, act)
            u = hp.features(X3[r], V3[r], L, 1.0)[1]
            refs.append((None, None, None, count[r] * ref[3], count[r] * ref[4]))
            scales.append(count[r] * hp.vjp_scales(W, cot3[r], u, N, L, 1.0)[2])
        worst = max(worst, _param_error(_np(g["g_W"]), _np(g["g_b"]), refs, scales))
    record_measure("pool_edges_multi_chunk_shared_params_vjp", worst)
    assert worst < hp.bound("vjp", N), worst
    env.close()


# ---- 2. v_scale and L ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
def test_v_scale_by_a_power_of_two_is_the_scaled_velocity(act):
    """u = (s V) 1 and u = V s have the same bits for s = +-2^n, so everything but g_v has, and g_v(s, V) = s g_v(1, s V)."""
    N, H = 1025, hp.SCALE_H
    X, V, W, b, cot = hp.scale_case(L, 1.0, N, H)
    env = _env(2, N)
    for s in hp.V_SCALES_EXACT:
        o1, g1 = env.pool(W, b, act, s, x=X, v=V), env.pool_vjp(W, b, cot, act, s, x=X, v=V)
        o2, g2 = env.pool(W, b, act, 1.0, x=X, v=s * V), env.pool_vjp(W, b, cot, act, 1.0, x=X, v=s * V)
        assert _same(o1, o2) and all(_same(g1[k], g2[k]) for k in ("g_x", "g_W", "g_b")), s
        assert _same(g1["g_v"], s * g2["g_v"]), s
        assert np.any(g1["g_v"] != 0)                              # (a g_v of zeros would show nothing)
    env.close()


@pytest.mark.parametrize("act", ACTS)
def test_v_scale_zero_is_the_zero_velocity(act):
    """u_max = 0: the relu unit without its velocity term, no velocity gradient and no gradient of W_k2."""
    N, H = 1025, hp.SCALE_H
    X, V, W, b, cot = hp.scale_case(L, 1.0, N, H)
    env = _env(2, N)
    o0, g0 = env.pool(W, b, act, 0.0, x=X, v=V), env.pool_vjp(W, b, cot, act, 0.0, x=X, v=V)
    oz, gz = env.pool(W, b, act, 1.0, x=X, v=0.0 * X), env.pool_vjp(W, b, cot, act, 1.0, x=X, v=0.0 * X)
    assert _same(o0, oz) and _same(g0["g_x"], gz["g_x"]) and _same(g0["g_W"][:, :2], gz["g_W"][:, :2]) and _same(g0["g_b"], gz["g_b"])
    assert np.all(g0["g_v"] == 0) and np.all(g0["g_W"][:, 2] == 0)
    assert np.any(o0 != 0) and np.any(g0["g_x"] != 0)
    ef, eg = hp.batch_errors(o0, {**g0, "g_v": None, "g_W": None, "g_b": None}, X, V, W, b, cot, L, act, 0.0)
    assert ef < hp.bound("forward", N) and eg < hp.bound("vjp", N), (ef, eg)
    env.close()


@pytest.mark.parametrize("N", hp.SCALE_NS)
@pytest.mark.parametrize("Lb", hp.BOX_LENGTHS)
def test_parity_at_other_v_scale_and_box_length(Lb, N):
    H = hp.SCALE_H
    env = _env_L(2, N, Lb)
    worst = {"forward": 0.0, "vjp": 0.0}
    for s, act in itertools.product(hp.V_SCALES, ACTS):
        assert (Lb, s, N, H) in hp.BOUND_SETS
        X, V, W, b, cot = hp.scale_case(Lb, s, N, H)
        Wp, bp = _per_env(W, b, 2)
        out, g = env.pool(Wp, bp, act, s, x=X, v=V), env.pool_vjp(Wp, bp, cot, act, s, x=X, v=V)
        ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, Lb, act, s)
        _measure(f"scale_L{Lb:.4g}_N{N}", worst, ef, eg)
        assert ef < hp.bound("forward", N) and eg < hp.bound("vjp", N), (s, act, ef, eg)
    env.close()


# ---- 3. N at a chunk's limits, H at the layer's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [3, 255, 256])
@pytest.mark.parametrize("N", [2, 3, 1023, 1024, 1025, 2047, 2048, 2049])
def test_parity_at_chunk_and_hidden_boundaries(N, H):
    """test_parity_with_the_longdouble_twin's check in a batch of two: shared and per-environment parameters, both activations."""
    E = 2
    X, V = _data(E, N, seed=N + H)
    sets = [_layer(H, seed=1), _layer(H, seed=2)]
    cot = np.random.default_rng(H).normal(0.0, 1.0, (E, H))
    env = _env(E, N)
    worst = {"forward": 0.0, "vjp": 0.0}
    for act in ACTS:
        refs = {}

        def ref(e, s):
            if (e, s) not in refs:
                u = hp.features(X[e], V[e], L, 1.0)[1]
                refs[e, s] = (hp.both_ld(X[e], V[e], *sets[s], cot[e], L, act), hp.vjp_scales(sets[s][0], cot[e], u, N, L, 1.0)[2])
            return refs[e, s]

        for per_env in (False, True):
            which = [1, 0] if per_env else [0, 0]
            W = np.stack([sets[s][0] for s in which]) if per_env else sets[0][0]
            b = np.stack([sets[s][1] for s in which]) if per_env else sets[0][1]
            out, g = env.pool(W, b, act, x=X, v=V), env.pool_vjp(W, b, cot, act, x=X, v=V)
            for e in range(E):
                ef, eg = _env_errors(out[e], g, e, ref(e, which[e])[0], X, V, *sets[which[e]], cot, act)
                if per_env:
                    eg = max(eg, _param_error(g["g_W"][e], g["g_b"][e], [ref(e, which[e])[0]], [ref(e, which[e])[1]]))
                _measure(f"boundary_N{N}_H{H}", worst, ef, eg)
            if not per_env:
                rs = [ref(e, 0) for e in range(E)]
                _measure(f"boundary_N{N}_H{H}", worst, 0.0, _param_error(g["g_W"], g["g_b"], [r[0] for r in rs], [r[1] for r in rs]))
    assert worst["forward"] < hp.bound("forward", N) and worst["vjp"] < hp.bound("vjp", N), worst
    env.close()


# ---- 4. the activations' edges ------------------------------------------------------------------------------------------------------
def _edge_setup():
    E, N, H = hp.EDGE_E, hp.EDGE_N, hp.EDGE_H
    X, V = hp.box_data(E, N, seed=23)
    W, b = hp.edge_layer()
    Wp, bp = _per_env(W, b, E)
    return E, N, H, X, V, Wp, bp, hp.edge_cot(), hp.bound("forward", N), hp.bound("vjp", N)


def test_relu_at_exactly_zero():
    """Row 0 = (0, 0, 1), -1 and u = 1.0 at half of the particles: z = 0 exactly, which is not > 0.  The others below 1
    (environment 0): out_0 and g_b_0 are +0; the others at u = 3 (environment 1): g_b_0 counts those alone, as the twin does --
    a >= would move it by cot_0 / 2."""
    E, N, H, X, _, Wp, bp, cot, fb, vb = _edge_setup()
    env = _env(E, N)
    worst = {"forward": 0.0, "vjp": 0.0}
    outs = []
    for scale in (1.0, 2.0):
        V, s = hp.kink_velocities(scale)
        assert np.all((V * s)[:, ::2] == 1.0) and np.all((V * s)[0, 1::2] < 1.0) and np.all((V * s)[1, 1::2] == 3.0)
        out, g = env.pool(Wp, bp, "relu", s, x=X, v=V), env.pool_vjp(Wp, bp, cot, "relu", s, x=X, v=V)
        ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, L, "relu", s)
        _measure("relu_kink", worst, ef, eg)
        assert ef < fb and eg < vb, (scale, ef, eg)
        assert _pos_zero(out[0, 0]) and _pos_zero(g["g_b"][0, 0]) and _pos_zero(g["g_W"][0, 0]), scale
        assert out[1, 0] != 0 and g["g_b"][1, 0] != 0
        outs.append(out)
    assert _same(*outs)
    env.close()


def test_tanh_saturated():
    """Row 1 has W_12 = 40: where |u| > 1 the unit is +-1 in float64 and 1 - h^2 = 0.  Environment 0 holds such particles
    only: out_1 is the mean of their signs, its parameter gradients are +0.  With W_12 = 1e200 and one v = 1e200, z = inf."""
    E, N, H, X, _, Wp, bp, cot, fb, vb = _edge_setup()
    env = _env(E, N)
    V = hp.saturating_velocities()
    out, g = env.pool(Wp, bp, "tanh", x=X, v=V), env.pool_vjp(Wp, bp, cot, "tanh", x=X, v=V)
    ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, L, "tanh")
    assert ef < fb and eg < vb, (ef, eg)
    assert _same(out[0, 1], np.float64(np.sum(np.sign(V[0]))) / N)
    assert _pos_zero(g["g_W"][0, 1]) and _pos_zero(g["g_b"][0, 1])
    Vh, Wh = V.copy(), Wp.copy()
    Vh[1, 5], Wh[:, 1, 2] = 1e200, 1e200
    outh = env.pool(Wh, bp, "tanh", x=X, v=Vh)
    eh = hp.batch_errors(outh, None, X, Vh, Wh, bp, None, L, "tanh")[0]
    _measure("tanh_saturated", {"forward": 0.0, "vjp": 0.0}, max(ef, eh), eg)
    assert np.isfinite(outh).all() and eh < fb, eh
    env.close()


def test_relu_zero_row_gives_plus_zero_and_leaves_the_others():
    """Row 2 is all zero, B_2 = 0: out_2, g_W_2. and g_b_2 are +0, and the other rows have the bits of the layer without it."""
    E, N, H, X, V, Wp, bp, cot, fb, vb = _edge_setup()
    env = _env(E, N)
    out, g = env.pool(Wp, bp, "relu", x=X, v=V), env.pool_vjp(Wp, bp, cot, "relu", x=X, v=V)
    ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, L, "relu")
    _measure("relu_zero_row", {"forward": 0.0, "vjp": 0.0}, ef, eg)
    assert ef < fb and eg < vb, (ef, eg)
    assert _pos_zero(out[:, 2]) and _pos_zero(g["g_W"][:, 2]) and _pos_zero(g["g_b"][:, 2])
    rest = [0, 1, 3, 4, 5]
    W5, b5, c5 = (np.ascontiguousarray(a[:, rest]) for a in (Wp, bp, cot))
    o5, g5 = env.pool(W5, b5, "relu", x=X, v=V), env.pool_vjp(W5, b5, c5, "relu", x=X, v=V)
    assert _same(out[:, rest], o5) and _same(g["g_W"][:, rest], g5["g_W"]) and _same(g["g_b"][:, rest], g5["g_b"])
    assert _same(g["g_x"], g5["g_x"]) and _same(g["g_v"], g5["g_v"])       # (the zero row adds +-0 to sums that start at +0)
    env.close()


def test_relu_bound_overflow_is_nan_in_its_row_alone():
    """v = 1e200 in environment 1 and W_32 = 1e200: B_3 is infinite there, out_3 is NaN; every other output is finite and
    within the bound of the twin at its scale max(1, B_k), which is about 1e200 in that environment.  Forward only."""
    E, N, H, X, V, Wp, bp, cot, fb, vb = _edge_setup()
    env = _env(E, N)
    Vh, Wh = V.copy(), Wp.copy()
    Vh[1, 5], Wh[:, 3, 2] = 1e200, 1e200
    clean = env.pool(Wp, bp, "relu", x=X, v=V)
    out = env.pool(Wh, bp, "relu", x=X, v=Vh)
    assert np.isnan(out[1, 3]) and np.isfinite(np.delete(out[1], 3)).all() and np.isfinite(out[0]).all()
    with np.errstate(over="ignore", invalid="ignore"):          # (the float64 B_3 of the scales is infinite, as the device's is)
        e0 = hp.batch_errors(out[:1], None, X[:1], Vh[:1], Wh[:1], bp[:1], None, L, "relu")[0]
        e1 = hp.batch_errors(out[1:], None, X[1:], Vh[1:], Wh[1:], bp[1:], None, L, "relu", skip=(3,))[0]
    _measure("relu_overflow", {"forward": 0.0, "vjp": 0.0}, max(e0, e1))
    assert e0 < fb and e1 < fb, (e0, e1)
    assert _same(env.pool(Wp, bp, "relu", x=X, v=V), clean)
    env.close()


# ---- 5. the NaN rule, row by row -----------------------------------------------------------------------------------------------------
def _nan_all(a):
    return bool(np.isnan(_np(a)).all())


@pytest.mark.parametrize("act", ACTS)
def test_nan_rule_row_by_row(act):
    E, N, H = 3, 1000, 5
    X, V = _data(E, N, seed=71)
    Ws, bs = _layer(H, seed=15)
    W, b = _per_env(Ws, bs, E)
    cot = np.random.default_rng(16).normal(0.0, 1.0, (E, H))
    env = _env(E, N)
    clean, gclean = env.pool(W, b, act, x=X, v=V), env.pool_vjp(W, b, cot, act, x=X, v=V)
    clean_s, gclean_s = env.pool(Ws, bs, act, x=X, v=V), env.pool_vjp(Ws, bs, cot, act, x=X, v=V)
    assert np.isfinite(clean).all() and all(np.isfinite(gclean[k]).all() for k in KEYS)

    def still_clean(why):          # the accumulators and the max words were cleared behind the poisoned read
        assert _same_results(clean, gclean, env.pool(W, b, act, x=X, v=V), env.pool_vjp(W, b, cot, act, x=X, v=V)), why

    def others_clean(out, g, why):
        for e in (0, 2):
            assert out is None or _same(out[e], clean[e]), (why, e)
            assert all(_same(g[k][e], gclean[k][e]) for k in KEYS), (why, e)

    # a non-finite row of parameters
    for where, k, bad in (("W", 2, np.nan), ("b", 4, np.inf)):
        Wb, bb = W.copy(), b.copy()
        if where == "W":
            Wb[1, k, 0] = bad
        else:
            bb[1, k] = bad
        out, g = env.pool(Wb, bb, act, x=X, v=V), env.pool_vjp(Wb, bb, cot, act, x=X, v=V)
        rest = [j for j in range(H) if j != k]
        assert np.isnan(out[1, k]) and _same(out[1, rest], clean[1, rest]), (where, k)
        assert _nan_all(g["g_W"][1, k]) and np.isnan(g["g_b"][1, k]), (where, k)
        others_clean(out, g, where)
        still_clean(where)
        # ... shared: the row is every environment's
        Wb, bb = Ws.copy(), bs.copy()
        if where == "W":
            Wb[k, 0] = bad
        else:
            bb[k] = bad
        out, g = env.pool(Wb, bb, act, x=X, v=V), env.pool_vjp(Wb, bb, cot, act, x=X, v=V)
        assert _nan_all(out[:, k]) and _same(out[:, rest], clean_s[:, rest]), (where, k, "shared")
        assert _nan_all(g["g_W"][k]) and np.isnan(g["g_b"][k]), (where, k, "shared")
        still_clean(where + ", shared")
    # a non-finite cotangent
    for bad in (np.inf, np.nan):
        cb = cot.copy()
        cb[1, 3] = bad
        g = env.pool_vjp(W, b, cb, act, x=X, v=V)
        rest = [j for j in range(H) if j != 3]
        assert _nan_all(g["g_W"][1, 3]) and np.isnan(g["g_b"][1, 3]), bad
        assert _same(g["g_W"][1, rest], gclean["g_W"][1, rest]) and _same(g["g_b"][1, rest], gclean["g_b"][1, rest]), bad
        others_clean(None, g, ("cot", bad))
        still_clean(("cot", bad))
    # a non-finite position
    for bad in (np.inf, np.nan):
        Xb = X.copy()
        Xb[1, 17] = bad
        out, g = env.pool(W, b, act, x=Xb, v=V), env.pool_vjp(W, b, cot, act, x=Xb, v=V)
        assert _nan_all(out[1]) and all(_nan_all(g[k][1]) for k in KEYS), bad
        others_clean(out, g, ("x", bad))
        still_clean(("x", bad))
        # ... shared parameters: the sum over the environments holds environment 1's NaN, the forward of the others does not
        out = env.pool(Ws, bs, act, x=Xb, v=V)
        assert _nan_all(out[1]) and _same(out[[0, 2]], clean_s[[0, 2]]), bad
        assert _same_results(clean_s, gclean_s, env.pool(Ws, bs, act, x=X, v=V), env.pool_vjp(Ws, bs, cot, act, x=X, v=V)), bad
    env.close()


# ---- 6. switched-off outputs and the torch op ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("per_env", [False, True])
def test_switched_off_outputs(per_env, device):
    E, N, H = 2, 1025, 5
    X, V = _data(E, N, seed=81)
    W, b = _layer(H, seed=19, lead=(E,) if per_env else ())
    cot = np.random.default_rng(20).normal(0.0, 1.0, (E, H))
    args = _cuda(W, b, cot, X, V) if device else [W, b, cot, X, V]
    env = _env(E, N)
    for act in ACTS:
        call = lambda **kw: env.pool_vjp(args[0], args[1], args[2], act, x=args[3], v=args[4], **kw)
        fwd = env.pool(args[0], args[1], act, x=args[3], v=args[4])
        full = call()
        for gx, gv, gp in itertools.product((False, True), repeat=3):
            g = call(g_x=gx, g_v=gv, g_params=gp)
            for k, on in (("g_x", gx), ("g_v", gv), ("g_W", gp), ("g_b", gp)):
                assert (g[k] is not None and _same(g[k], full[k])) if on else g[k] is None, (act, gx, gv, gp, k)
            if not (gx or gv or gp):       # nothing was enqueued, and the work block is as a forward needs it
                assert _same(env.pool(args[0], args[1], act, x=args[3], v=args[4]), fwd), act
    env.close()


@pytest.mark.parametrize("per_env", [False, True])
def test_torch_op_routes_the_gradients_that_are_needed(per_env):
    from ocplasma_amd.control.pool import pooled_features
    E, N, H, s = 2, 1025, 5, 0.37
    X, V = _data(E, N, seed=91)
    W, b = _layer(H, seed=21, lead=(E,) if per_env else ())
    cot = np.random.default_rng(22).normal(0.0, 1.0, (E, H))
    env = _env(E, N)
    base = _cuda(X, V, W, b)
    tc = _cuda(cot)[0]
    for act in ACTS:
        want = env.pool_vjp(base[2], base[3], tc, act, s, x=base[0], v=base[1])
        fwd = env.pool(base[2], base[3], act, s, x=base[0], v=base[1])
        for need in [(0,), (1,), (2,), (3,), (0, 1, 2, 3)]:
            t = [a.clone().requires_grad_(i in need) for i, a in enumerate(base)]
            out = pooled_features(env, *t, act, s)
            assert _same(out, fwd), (act, need)
            out.backward(tc)
            for i, k in enumerate(KEYS):
                if i in need:
                    assert t[i].grad is not None and _same(t[i].grad, want[k]), (act, need, k)
                else:
                    assert t[i].grad is None, (act, need, k)
    env.close()


# ---- 7. one handle, changing shapes -----------------------------------------------------------------------------------------------------
#            H  vjp    per_env device stored poison
SEQUENCE = [(64, False, False, False, False, False),
            (256, True, True, True, True, False),        # the large VJP: 3 x 1024 sums ...
            (1, False, False, False, False, False),      # ... a small host forward puts its copies of x, v, params where they were
            (256, True, False, True, False, False),      # ... and the large VJP again
            (1, True, True, False, True, False),
            (64, False, True, True, False, True),        # a non-finite position in environment 1
            (256, False, False, False, True, False),
            (64, True, False, False, False, True),
            (1, False, True, True, False, False),
            (256, True, True, False, False, False),
            (1, False, False, False, True, False),
            (256, True, False, True, True, False),
            (64, True, True, True, False, False)]


def test_one_handle_through_calls_of_changing_shape():
    """Every call of the sequence on one handle equals the same call on a fresh handle bit for bit: the work block's sums are
    zero at every call, wherever the calls before put their copies and whatever their H, kind and memory were."""
    E, N = 3, 1025
    Xs, Vs = _data(E, N, seed=101)
    Xg, Vg = _data(E, N, seed=102)
    Xbad = Xg.copy()
    Xbad[1, 17] = np.inf

    def make():
        env = _env(E, N)
        env.reset(Xs, Vs)
        return env

    def run(env, i, H, vjp, per_env, device, stored, poison):
        act = ACTS[i % 2]
        W, b = _layer(H, seed=30 + i, lead=(E,) if per_env else ())
        cot = np.random.default_rng(60 + i).normal(0.0, 1.0, (E, H))
        x, v = (None, None) if stored else (Xbad if poison else Xg, Vg)
        if device:
            W, b, cot = _cuda(W, b, cot)
            x, v = (None, None) if stored else _cuda(x, v)
        if vjp:
            g = env.pool_vjp(W, b, cot, act, x=x, v=v, on_device=device)
            return [g[k] for k in KEYS]
        return [env.pool(W, b, act, x=x, v=v, on_device=device)]

    assert len(SEQUENCE) >= 10
    env = make()
    got = [run(env, i, *c) for i, c in enumerate(SEQUENCE)]
    env.close()
    for i, c in enumerate(SEQUENCE):
        fresh = make()
        want = run(fresh, i, *c)
        fresh.close()
        assert len(want) == len(got[i]) and all(_same(a, w) for a, w in zip(got[i], want)), (i, c)
        if c[5]:
            assert all(_nan_all(a[1]) for a in got[i][:2]), (i, c)
        else:
            assert all(np.isfinite(_np(a)).all() for a in got[i]), (i, c)
