"""Forward mode of the pooled particle features on the device (pic_pool_jvp, pic_pool_ln_jvp, BatchedPIC.pool_jvp,
pooled_features(forward_ad=True)): parity with the float64 restatement of tests/hp_pool_jvp.py over the grid, what
must hold bit for bit, duality with the device's VJP, central differences of the device's forward, the edges the contract
defines, the refusals by message, the torch op under forward_ad and torch.func.jvp, and the closed loop through
rollout_policy_jvp(observe="state")."""
import itertools

import numpy as np
import pytest
import torch

import hp_pool as hp
import hp_pool_jvp as hj
import hp_pool_ln as hpl
from conftest import record_measure
from test_gpu_pool import _cuda, _np, _same  # noqa: F401

pytestmark = pytest.mark.gpu

L = hj.L
ACTS = hj.ACTS
LAYERS = (False, True)                  # ln


def _env(E, N, Ng=64, L_=L, **kw):
    from ocplasma_amd.env.batched import BatchedPIC
    return BatchedPIC(E, N, Ng, L=L_, dt=0.1, **kw)


def _p(p, ln):
    """pool_jvp's parameter arguments of a (W, b, gamma, beta) set."""
    return dict(gamma=p[2], beta=p[3]) if ln else {}


def _t(t, ln):
    """... and the tangents of the layer at hand out of a dict that may hold the LayerNorm's too."""
    return {k: a for k, a in t.items() if ln or k not in ("d_gamma", "d_beta")}


def _jvp(env, p, act, ln, x=None, v=None, **t):
    return env.pool_jvp(p[0], p[1], activation=act, x=x, v=v, **_p(p, ln), **_t(t, ln))


def _case(E, N, H, seed, K=None, lead=False):
    """X, V [E, N], a (W, b, gamma, beta) set (per environment with lead), cot [E, H] and tangents of every input."""
    X, V = hp.box_data(E, N, seed=seed)
    p = hpl.layer(H, seed=seed + 1, lead=(E,) if lead else ())
    rng = np.random.default_rng(seed + 2)
    k = () if K is None else (K,)
    pl = k + ((E,) if lead else ())
    t = {"d_x": rng.normal(0.0, 1.0, k + (E, N)), "d_v": rng.normal(0.0, 1.0, k + (E, N)), "d_W": rng.normal(0.0, 1.0, pl + (H, 3)),
         "d_b": rng.normal(0.0, 1.0, pl + (H,)), "d_gamma": rng.normal(0.0, 1.0, pl + (H,)), "d_beta": rng.normal(0.0, 1.0, pl + (H,))}
    return X, V, p, rng.normal(0.0, 1.0, (E, H)), t


# ---- 1. parity with the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", hj.GRID_H)
@pytest.mark.parametrize("N", hj.GRID_N)
def test_parity_with_the_restatement(N, H):
    """Every direction of a call against the float64 restatement, relative to each output's contract bound, for relu and tanh,
    shared and per-environment parameters, both layers, in a batch of three and alone, with K = hj.grid_K(N, H) directions (8, 3
    or 1).  The stored-particle, host-memory and device-memory forms must agree bit for bit."""
    X, V, sets, _ = hpl.grid_case(N, H)
    dX, dV, tsets = hj.grid_tangents(N, H)
    K = hj.grid_K(N, H)
    env3, env1 = _env(3, N), _env(1, N)
    worst = {False: 0.0, True: 0.0}
    for env, E in ((env3, 3), (env1, 1)):
        env.reset(X[:E], V[:E])
        Xs, Vs = env.particles()
        for act, per_env, ln in itertools.product(ACTS, (False, True), LAYERS):
            which = [1, 0, 0][:E] if per_env else [0] * E
            p = tuple(np.stack([sets[s][i] for s in which]) for i in range(4)) if per_env else sets[0]
            t = {k: (np.stack([tsets[s][k][:K] for s in which], axis=1) if per_env else tsets[0][k][:K]) for k in hj.PARAM_T[ln]}
            t["d_x"], t["d_v"] = dX[:K, :E], dV[:K, :E]
            x, v = X[:E], V[:E]
            out = _jvp(env, p, act, ln, x, v, **t)
            assert out.shape == (K, E, H)
            for kk, (e, s) in itertools.product(range(K), enumerate(which)):
                want, B = hj.grid_restated(N, H, e, s, act, ln, kk)
                worst[ln] = max(worst[ln], hj.rel_error(out[kk, e], want, B))
            tp, (tx, tv) = _cuda(*p), _cuda(x, v)
            tt = dict(zip(t, _cuda(*t.values())))
            assert _same(out, _jvp(env, tp, act, ln, tx, tv, **tt)), (act, E, per_env, ln, "device")
            so = _jvp(env, p, act, ln, Xs, Vs, **t)
            assert _same(so, _jvp(env, p, act, ln, **t)), (act, E, per_env, ln, "stored, host")
            assert _same(so, _jvp(env, tp, act, ln, **tt)), (act, E, per_env, ln, "stored, device")
            if np.array_equal(Xs, x) and np.array_equal(Vs, v):
                assert _same(out, so)
    for ln in LAYERS:
        record_measure(f"pool_jvp_parity_{'ln' if ln else 'plain'}_N{N}_H{H}", worst[ln])
    print(f"pool_jvp parity N={N} H={H} K={K}: plain {worst[False]:.3e} (bound {hj.bound(False, N):.3e}) "
          f"ln {worst[True]:.3e} (bound {hj.bound(True, N):.3e})")
    assert worst[False] < hj.bound(False, N) and worst[True] < hj.bound(True, N), worst
    env3.close()
    env1.close()


@pytest.mark.parametrize("ln", LAYERS)
def test_each_tangent_alone_and_none_at_all(ln):
    """d_x, d_v and the parameters' tangents each alone non-NULL against the restatement; all NULL gives exactly +0."""
    E, N, H, K = 2, 1025, 5, 3
    X, V, p, _, t = _case(E, N, H, seed=11, K=K)
    env = _env(E, N)
    for act in ACTS:
        for keys in (("d_x",), ("d_v",), hj.PARAM_T[ln], ("d_b",)):
            sub = {k: t[k] for k in keys}
            out = _jvp(env, p, act, ln, X, V, **sub)
            want, B = hj.restated(X, V, p[0], p[1], L, act, **_p(p, ln), **sub)
            err = max(hj.rel_error(out[kk, e], want[kk, e], B[kk, e]) for kk in range(K) for e in range(E))
            record_measure(f"pool_jvp_alone_{'ln' if ln else 'plain'}_{act}_{keys[0]}", err)
            assert err < hj.bound(ln, N), (act, keys, err)
        for on_device in (False, True):
            zero = env.pool_jvp(p[0], p[1], activation=act, x=X, v=V, on_device=on_device, **_p(p, ln))
            assert zero.shape == (E, H) and _same(zero, np.zeros((E, H))), act          # (+0: the bits)
    env.close()


# ---- 2. bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", LAYERS)
def test_results_do_not_depend_on_directions_order_batch_geometry_or_run(ln):
    act = "relu" if ln else "tanh"
    E, N, H, K = 2, 4097, 5, 8
    X, V, p, _, t = _case(E, N, H, seed=21, K=K)
    env = _env(E, N)
    out = _jvp(env, p, act, ln, X, V, **t)
    assert _same(out, _jvp(env, p, act, ln, X, V, **t))                                  # two runs
    for kk in range(K):                                                                  # K directions in one call against K calls
        one = _jvp(env, p, act, ln, X, V, **{k: a[kk] for k, a in t.items()})
        assert one.shape == (E, H) and _same(one, out[kk]), kk
    assert _same(out[2:5], _jvp(env, p, act, ln, X, V, **{k: a[2:5] for k, a in t.items()}))
    perm = np.random.default_rng(6).permutation(N)                                       # the particles of environment 1 permuted
    Xp, Vp, tp = X.copy(), V.copy(), {k: a.copy() for k, a in t.items()}
    Xp[1], Vp[1] = X[1][perm], V[1][perm]
    tp["d_x"][:, 1], tp["d_v"][:, 1] = t["d_x"][:, 1][:, perm], t["d_v"][:, 1][:, perm]
    assert _same(out, _jvp(env, p, act, ln, Xp, Vp, **tp))
    env.close()
    for bpe in (1, 7):                                                                   # another launch geometry of the handle
        other = _env(E, N, blocks_per_env=bpe)
        assert _same(out, _jvp(other, p, act, ln, X, V, **t)), bpe
        other.close()
    # environment 1 alone, and at row 299 of a batch of 300 (per-environment parameters and tangents)
    K2 = 3
    t2 = {k: a[:K2] for k, a in t.items()}
    rep = lambda a, n: np.broadcast_to(a, (n,) + a.shape).copy()                         # noqa: E731
    reps = lambda a, n: np.broadcast_to(a[:, None], (K2, n) + a.shape[1:]).copy()        # noqa: E731
    big = _env(300, N)
    Xb, Vb = np.tile(X[0], (300, 1)), np.tile(V[0], (300, 1))
    Xb[299], Vb[299] = X[1], V[1]
    tb = {k: (np.tile(a[:, :1], (1, 300, 1)) if k in ("d_x", "d_v") else reps(a, 300)) for k, a in t2.items()}
    tb["d_x"][:, 299], tb["d_v"][:, 299] = t2["d_x"][:, 1], t2["d_v"][:, 1]
    ob = _jvp(big, tuple(rep(a, 300) for a in p), act, ln, Xb, Vb, **tb)
    big.close()
    one = _env(1, N)
    t1 = {k: (a[:, 1:] if k in ("d_x", "d_v") else reps(a, 1)) for k, a in t2.items()}
    o1 = _jvp(one, tuple(a[None] for a in p), act, ln, X[1:], V[1:], **t1)
    one.close()
    assert _same(o1[:, 0], ob[:, 299]) and _same(o1[:, 0], out[:K2, 1]) and _same(ob[:, 0], out[:K2, 0])


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2049])
def test_chunk_boundaries(N):
    """Around one and two chunks of 1024 particles: against the restatement, and K directions against K calls, both layers."""
    E, H, K = 2, 3, 2
    X, V, p, _, t = _case(E, N, H, seed=N, K=K)
    env = _env(E, N)
    for ln in LAYERS:
        out = _jvp(env, p, "tanh", ln, X, V, **t)
        want, B = hj.restated(X, V, p[0], p[1], L, "tanh", **_p(p, ln), **_t(t, ln))
        err = max(hj.rel_error(out[kk, e], want[kk, e], B[kk, e]) for kk in range(K) for e in range(E))
        assert err < hj.bound(ln, N), (ln, err)
        for kk in range(K):
            assert _same(out[kk], _jvp(env, p, "tanh", ln, X, V, **{k: a[kk] for k, a in t.items()})), (ln, kk)
    env.close()


def test_two_chunks_per_workgroup_match_a_one_environment_handle():
    """4096 x 1025 at H = 3, K = 2: two chunks per workgroup, against a handle of one environment."""
    E, N, H, K = 4096, 1025, 3, 2
    assert hp.plan(E, N)["chunks_per_wg"] == 2 and hp.plan(1, N)["chunks_per_wg"] == 1
    X, V, p, _, t = _case(2, N, H, seed=33, K=K)
    rep = lambda a: np.broadcast_to(a, (E,) + a.shape).copy()                             # noqa: E731
    Xb, Vb = np.tile(X[0], (E, 1)), np.tile(V[0], (E, 1))
    Xb[E - 1], Vb[E - 1] = X[1], V[1]
    tb = {k: (np.tile(a[:, :1], (1, E, 1)) if k in ("d_x", "d_v") else np.broadcast_to(a[:, None], (K, E) + a.shape[1:]).copy())
          for k, a in t.items()}
    tb["d_x"][:, E - 1], tb["d_v"][:, E - 1] = t["d_x"][:, 1], t["d_v"][:, 1]
    big, one = _env(E, N), _env(1, N)
    for ln in LAYERS:
        ob = _jvp(big, tuple(rep(a) for a in p), "relu", ln, Xb, Vb, **tb)
        for row, e in ((0, 0), (E - 1, 1)):
            t1 = {k: (a[:, e:e + 1] if k in ("d_x", "d_v") else a[:, None]) for k, a in t.items()}
            o1 = _jvp(one, tuple(a[None] for a in p), "relu", ln, X[e:e + 1], V[e:e + 1], **t1)
            assert _same(o1[:, 0], ob[:, row]), (ln, row)
    big.close()
    one.close()


# ---- 3. duality and central differences ---------------------------------------------------------------------------------------------
DUALITY_SHAPES = ((1025, 5), (4097, 64))


def _duality_floor():
    """The largest gap of the two float64 restatements (hp_pool_jvp.duality_gap) at the shapes of the device's duality test."""
    worst = 0.0
    for N, H in DUALITY_SHAPES:
        X, V, p, cot, t = _case(2, N, H, seed=N + H, lead=True)
        for ln, act, e in itertools.product(LAYERS, ACTS, range(2)):
            te = {k: a[e] for k, a in _t(t, ln).items()}
            kw = dict(gamma=p[2][e], beta=p[3][e]) if ln else {}
            worst = max(worst, hj.duality_gap(X[e], V[e], p[0][e], p[1][e], cot[e], L, act, **kw, **te))
    return worst


def test_duality_with_the_device_vjp():
    """<cot, pool_jvp> against <pool_vjp, tangents> per environment, relative to sum_k |cot_k| B_k.  Bound: 100 x the largest gap
    of the two restatements on the CPU at the same shapes (measured 1.4e-16; the rule of DESIGN.md 7c)."""
    floor = _duality_floor()
    record_measure("pool_jvp_duality_restatements", floor)
    worst = 0.0
    for N, H in DUALITY_SHAPES:
        X, V, p, cot, t = _case(2, N, H, seed=N + H, lead=True)
        env = _env(2, N)
        for ln, act in itertools.product(LAYERS, ACTS):
            tt = _t(t, ln)
            out = _jvp(env, p, act, ln, X, V, **tt)
            g = env.pool_vjp(p[0], p[1], cot, act, x=X, v=V, **_p(p, ln))
            _, B = hj.restated(X, V, p[0], p[1], L, act, **_p(p, ln), **{k: a[None] for k, a in tt.items()})
            for e in range(2):
                lhs = float(np.dot(cot[e], out[e]))
                rhs = sum(float(np.sum(g["g_" + k[2:]][e] * a[e])) for k, a in tt.items())
                gap = abs(lhs - rhs) / float(np.sum(np.abs(cot[e]) * B[0, e]))
                worst = max(worst, gap)
                assert gap < 100.0 * floor, (N, H, ln, act, e, gap, floor)
        env.close()
    record_measure("pool_jvp_duality_device", worst)


def test_central_differences_of_the_device_forward():
    """<cot, pool_jvp> against (f(theta + h d) - f(theta - h d)) / 2h of the device's forward along d, relative to
    sum_k |cot_k| B_k, within 100 x the same figure of the restatements (its jvp against the restated forward's difference)."""
    E, N, H, h = 2, 1000, 5, 1e-6
    X, V, p, cot, t = _case(E, N, H, seed=61, lead=True)
    env = _env(E, N)
    for ln, act in itertools.product(LAYERS, ACTS):
        tt = _t(t, ln)
        names = ("d_W", "d_b") + (("d_gamma", "d_beta") if ln else ())
        pp = p if ln else p[:2]
        moved = lambda s: (X + s * h * t["d_x"], V + s * h * t["d_v"], [a + s * h * t[k] for a, k in zip(pp, names)])     # noqa: E731

        def fwd_dev(s):
            x, v, q = moved(s)
            return env.pool(q[0], q[1], act, x=x, v=v, **(dict(gamma=q[2], beta=q[3]) if ln else {}))

        def fwd_cpu(s):
            x, v, q = moved(s)
            f = (lambda e: hpl.forward(x[e], v[e], *(a[e] for a in q), L, act)) if ln else \
                (lambda e: hp.forward(x[e], v[e], q[0][e], q[1][e], L, act))
            return np.stack([f(e) for e in range(E)])

        out = _jvp(env, p, act, ln, X, V, **tt)
        want, B = hj.restated(X, V, p[0], p[1], L, act, **_p(p, ln), **{k: a[None] for k, a in tt.items()})
        S = np.sum(np.abs(cot) * B[0], axis=1)
        fd = lambda f: np.sum(cot * (f(1.0) - f(-1.0)), axis=1) / (2.0 * h)                                              # noqa: E731
        own = float(np.max(np.abs(np.sum(cot * want[0], axis=1) - fd(fwd_cpu)) / S))
        dev = float(np.max(np.abs(np.sum(cot * out, axis=1) - fd(fwd_dev)) / S))
        record_measure(f"pool_jvp_fd_{'ln' if ln else 'plain'}_{act}_restatement", own)
        record_measure(f"pool_jvp_fd_{'ln' if ln else 'plain'}_{act}_device", dev)
        assert dev < 100.0 * own, (ln, act, dev, own)
    env.close()


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", LAYERS)
def test_non_finite_input_poisons_what_the_contract_says_and_nothing_else(ln):
    E, N, H, K = 3, 1000, 5, 3
    X, V, p, _, t = _case(E, N, H, seed=41, K=K, lead=True)
    t = _t(t, ln)
    env = _env(E, N)
    for act in ACTS:
        clean = _jvp(env, p, act, ln, X, V, **t)
        assert np.isfinite(clean).all()

        def check(out, nan, what):
            """`nan` [K, E, H] marks what must be NaN; everything else, and the next call, is bit for bit the clean result."""
            assert np.isnan(out[nan]).all() and _same(out[~nan], clean[~nan]), (act, what)
            assert _same(clean, _jvp(env, p, act, ln, X, V, **t)), (act, what)

        def mark(k=slice(None), e=slice(None), h=slice(None)):
            m = np.zeros((K, E, H), bool)
            m[k, e, h] = True
            return m

        def with_(name, idx, value, base=None):
            a = (t[name] if base is None else base).copy()
            a[idx] = value
            return a

        # a non-finite u or q: every direction of that environment
        for what, Xb, Vb in (("v inf", X, with_(None, (1, 17), np.inf, V)), ("x nan", with_(None, (1, N - 1), np.nan, X), V)):
            check(_jvp(env, p, act, ln, Xb, Vb, **t), mark(e=1), what)
        # v = 1e300: finite in the plain layer, NaN (the overflow rule) with the LayerNorm
        out = _jvp(env, p, act, ln, X, with_(None, (1, 17), 1e300, V), **t)
        if ln:
            check(out, mark(e=1), "v 1e300")
        else:
            assert np.isfinite(out).all() and _same(out[:, [0, 2]], clean[:, [0, 2]]), act
        # a non-finite tq or tu: that (direction, environment)
        for name, val in (("d_x", np.nan), ("d_x", np.inf), ("d_v", -np.inf)):
            check(_jvp(env, p, act, ln, X, V, **{**t, name: with_(name, (1, 2, 5), val)}), mark(k=1, e=2), name)
        # a non-finite dW_k. or db_k: d_out_k of that direction (plain), the direction of that environment (LayerNorm)
        for name, idx in (("d_W", (2, 0, 3, 1)), ("d_b", (2, 0, 3))):
            check(_jvp(env, p, act, ln, X, V, **{**t, name: with_(name, idx, np.nan)}),
                  mark(k=2, e=0) if ln else mark(k=2, e=0, h=3), name)
        # a non-finite W_k. or b_k: d_out_k in every direction (plain), the environment (LayerNorm)
        for i, idx in ((0, (1, 3, 2)), (1, (1, 3))):
            pw = tuple(with_(None, idx, np.inf, a) if j == i else a for j, a in enumerate(p))
            check(_jvp(env, pw, act, ln, X, V, **t), mark(e=1) if ln else mark(e=1, h=3), ("W", "b")[i])
        if ln:                                              # gamma_k, beta_k, dgamma_k, dbeta_k: d_out_k alone
            for i in (2, 3):
                pw = tuple(with_(None, (1, 3), np.nan, a) if j == i else a for j, a in enumerate(p))
                check(_jvp(env, pw, act, ln, X, V, **t), mark(e=1, h=3), ("gamma", "beta")[i - 2])
            for name in ("d_gamma", "d_beta"):
                check(_jvp(env, p, act, ln, X, V, **{**t, name: with_(name, (0, 1, 3), np.inf)}), mark(k=0, e=1, h=3), name)
    env.close()


@pytest.mark.parametrize("ln", LAYERS)
def test_powers_of_two_zero_bounds_and_one_hidden_unit(ln):
    E, N, H, K = 2, 1000, 5, 4
    X, V, p, _, t = _case(E, N, H, seed=43, K=K)
    t = _t(t, ln)
    env = _env(E, N)
    for act in ACTS:
        base = _jvp(env, p, act, ln, X, V, **t)
        # direction kk scaled by 2^300, 2^-300, 0, 1: the result's bits scale by exactly that factor
        scale = np.array([2.0 ** 300, 2.0 ** -300, 0.0, 1.0])
        ts = {k: a * scale.reshape((K,) + (1,) * (a.ndim - 1)) for k, a in t.items()}
        out = _jvp(env, p, act, ln, X, V, **ts)
        for kk in range(K):
            assert _same(out[kk], base[kk] * scale[kk] + 0.0), (act, kk)
        assert not np.signbit(out[2]).any()
        # a unit whose bound is zero (its row of W, dW and db zero; with the LayerNorm gamma_k, dgamma_k, dbeta_k zero): +0
        pz, tz = [a.copy() for a in p], {k: a.copy() for k, a in t.items()}
        if ln:
            pz[2][2] = 0.0
            tz["d_gamma"][:, 2] = tz["d_beta"][:, 2] = 0.0
        else:
            pz[0][2] = 0.0
            tz["d_W"][:, 2] = 0.0
            tz["d_b"][:, 2] = 0.0
        oz = _jvp(env, pz, act, ln, X, V, **tz)
        assert _same(oz[:, :, 2], np.zeros((K, E))) and np.isfinite(oz).all(), act
    if ln:
        # H = 1: y = 0 and every dy is +0, so the term is exactly a dbeta: d_out = dbeta mean_i a_i with a from act(beta), up to the
        # integer unit (and tanh's libm), which hj.bound holds relative to the output's bound
        p1 = hpl.layer(1, seed=5)
        t1 = {k: (a if k in ("d_x", "d_v") else a[:, :1]) for k, a in t.items()}
        _, B = hj.restated(X, V, p1[0], p1[1], L, "relu", **_p(p1, ln), **t1)
        for act, a in (("relu", 1.0 if p1[3][0] > 0 else 0.0), ("tanh", 1.0 - np.tanh(p1[3][0]) ** 2)):
            o1 = _jvp(env, p1, act, ln, X, V, **t1)
            assert np.max(np.abs(o1 - a * t1["d_beta"][:, None, :]) / B) < hj.bound(ln, N), act
    env.close()


def test_alternating_calls_share_the_block():
    """One handle through plain / LayerNorm, forward / VJP / JVP calls of changing H and K against fresh handles."""
    E, N = 2, 1025
    calls = [("jvp", True, 5, 3), ("fwd", False, 64, 0), ("jvp", False, 64, 8), ("vjp", True, 64, 0), ("jvp", True, 256, 1),
             ("jvp", False, 3, 5), ("vjp", False, 256, 0), ("jvp", True, 1, 8), ("fwd", True, 5, 0), ("jvp", False, 5, 2)]
    env = _env(E, N)
    for i, (kind, ln, H, K) in enumerate(calls):
        X, V, p, cot, t = _case(E, N, H, seed=70 + i, K=K or None)
        fresh = _env(E, N)
        res = []
        for e_ in (env, fresh):
            if kind == "jvp":
                res.append(_jvp(e_, p, "relu", ln, X, V, **t))
            elif kind == "fwd":
                res.append(e_.pool(p[0], p[1], "relu", x=X, v=V, **_p(p, ln)))
            else:
                g = e_.pool_vjp(p[0], p[1], cot, "relu", x=X, v=V, **_p(p, ln))
                res.append(np.concatenate([np.ravel(g[k]) for k in sorted(g)]))
        fresh.close()
        assert _same(res[0], res[1]), (i, kind, ln, H, K)
    env.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from ocplasma_amd import _abi
    E, N, H = 2, 100, 4
    env = _env(E, N)
    X, V = hp.box_data(E, N, seed=51)
    p = np.zeros(6 * H)
    out, dx = np.zeros((8, E, H)), np.zeros((8, E, N))
    A = lambda a: a.ctypes.data                                                          # noqa: E731
    H_ = _abi.PIC_HOST

    def both(why, x=A(X), v=A(V), K=1, kind=H_, d_out=A(out), **kw):
        plain = dict(hidden=H, activation=0, per_env=0, params_mem_kind=H_, v_scale=1.0, params=A(p))
        plain.update({k: a for k, a in kw.items() if k not in ("eps", "period")})
        full = dict(plain, eps=kw.get("eps", 1e-5), period=kw.get("period", 0.0))
        with pytest.raises(_abi.PicError, match=why):
            env._h.pool_jvp(_abi.PicPoolSpec(**plain), x, v, K, A(dx), 0, 0, kind, d_out)
        with pytest.raises(_abi.PicError, match=why):
            env._h.pool_ln_jvp(_abi.PicPoolLnSpec(**full), x, v, K, A(dx), 0, 0, kind, d_out)

    for K in (0, 9, -1):
        both(r"error -1: pic_pool_(ln_)?jvp: need 1 <= K <= 8", K=K)
    both(r"error -1: pic_pool_(ln_)?jvp: hidden must be 1\.\.256", hidden=0)
    both(r"error -1: pic_pool_(ln_)?jvp: hidden must be 1\.\.256", hidden=257)
    both(r"error -1: pic_pool_(ln_)?jvp: activation must be", activation=2)
    both(r"error -1: pic_pool_(ln_)?jvp: per_env must be 0 or 1", per_env=2)
    both(r"error -1: pic_pool_(ln_)?jvp: bad params_mem_kind", params_mem_kind=7)
    both(r"error -1: pic_pool_(ln_)?jvp: params is NULL", params=None)
    both(r"error -1: pic_pool_(ln_)?jvp: v_scale is not finite", v_scale=float("nan"))
    both(r"error -1: pic_pool_(ln_)?jvp: bad mem_kind", kind=5)
    both(r"error -1: pic_pool_(ln_)?jvp: x and v must both be given or both be NULL", v=0)
    both(r"error -1: pic_pool_(ln_)?jvp: d_out is NULL", d_out=0)
    with pytest.raises(_abi.PicError, match="error -1: pic_pool_ln_jvp: eps must be finite and > 0"):
        env._h.pool_ln_jvp(_abi.PicPoolLnSpec(H, 0, 0, H_, 1.0, 0.0, 0.0, A(p)), A(X), A(V), 1, 0, 0, 0, H_, A(out))
    with pytest.raises(_abi.PicError, match="error -1: pic_pool_ln_jvp: period must be finite and >= 0"):
        env._h.pool_ln_jvp(_abi.PicPoolLnSpec(H, 0, 0, H_, 1.0, 1e-5, -1.0, A(p)), A(X), A(V), 1, 0, 0, 0, H_, A(out))
    both(r"error -3: pic_pool_(ln_)?jvp: call pic_reset first", x=0, v=0)
    env.reset(X, V)
    env._h.pool_jvp(_abi.PicPoolSpec(H, 0, 0, H_, 1.0, A(p)), 0, 0, 8, A(dx), 0, 0, H_, A(out))      # (a refusal leaves the handle usable)
    assert not out.any()                                                                 # (zero parameters: a zero bound)
    env.close()
    env = _env(E, N, dtype="float32")
    env.reset(X, V)
    both(r"error -1: pic_pool_(ln_)?jvp: the stored particles need float64 particles with float64 positions", x=0, v=0)
    env.close()


# ---- 6. the torch op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", LAYERS)
def test_the_op_with_forward_ad(ln):
    """pooled_features(forward_ad=True): the default op's forward and backward bits, and tangents under
    torch.autograd.forward_ad and torch.func.jvp that are pool_jvp's bits; the default op still raises torch's own error."""
    import torch.autograd.forward_ad as fwAD
    from ocplasma_amd.control.pool import pooled_features
    E, N, H = 2, 1025, 5
    X, V, p, cot, t = _case(E, N, H, seed=81)
    p, names = (p if ln else p[:2]), ("d_x", "d_v") + hj.PARAM_T[ln]
    env = _env(E, N)
    env.use_torch_stream()
    want = _jvp(env, p + (None,) * (4 - len(p)), "relu", ln, X, V, **_t(t, ln))
    op = lambda a, fa: pooled_features(env, a[0], a[1], a[2], a[3], "relu", 1.0, *a[4:6], forward_ad=fa)     # noqa: E731
    res = []
    for fa in (False, True):
        a = [torch.tensor(x, device="cuda", requires_grad=True) for x in (X, V) + tuple(p)]
        out = op(a, fa)
        out.backward(torch.as_tensor(cot, device="cuda"))
        res.append([out.detach()] + [x.grad for x in a])
    assert all(_same(x, y) for x, y in zip(*res))
    prim = _cuda(X, V, *p)
    tang = _cuda(*(t[k] for k in names))
    with fwAD.dual_level():
        got = fwAD.unpack_dual(op([fwAD.make_dual(x, d) for x, d in zip(prim, tang)], True))
        assert _same(got.primal, res[0][0]) and _same(got.tangent, want)
        only_v = fwAD.unpack_dual(op([prim[0], fwAD.make_dual(prim[1], tang[1])] + prim[2:], True)).tangent     # (the others None)
        assert _same(only_v, env.pool_jvp(p[0], p[1], activation="relu", x=X, v=V, d_v=t["d_v"], **_p(p + (None,) * 2, ln)))
        with pytest.raises(NotImplementedError, match="forward mode AD"):
            op([fwAD.make_dual(x, d) for x, d in zip(prim, tang)], False)
    out, tan = torch.func.jvp(lambda *a: op(list(a), True), tuple(prim), tuple(tang))
    assert _same(out, res[0][0]) and _same(tan, want)
    env.close()


# ---- 7. the closed loop -----------------------------------------------------------------------------------------------------------------
def test_rollout_policy_jvp_through_the_op_is_dual_to_the_backward_and_matches_torch_layers():
    """rollout_policy_jvp(observe="state") under head(rho(pooled_features(forward_ad=True))) with a LayerNorm, at the shape of
    test_rollout_policy_jvp_is_dual_to_rollout_policy_backward: dual to rollout_policy's backward through the same op within its
    DUALITY_BOUND, and the tangents of the same policy written in float64 torch layers within test_gpu_policy_grad's bound."""
    from ocplasma_amd.control.pool import pooled_features
    from ocplasma_amd.env import grad
    from test_gpu_policy_grad import GRAD_BOUND
    from test_gpu_tangent_walk import DUALITY_BOUND, M, _make
    E, N, Ng, T, K, H, Ho = 3, 1000, 64, 5, 2, 8, 6
    env, X, V = _make(E, N, Ng, seed=6)
    env.use_torch_stream()
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                     # noqa: E731
    p0 = {"W": r(H, 3) * 0.5, "b": r(H) * 0.1, "gamma": 1.0 + 0.3 * r(H), "beta": 0.3 * r(H), "W2": r(Ho, H) * 0.5, "b2": r(Ho) * 0.1,
          "W3": r(2 * M, Ho) * 0.5, "b3": r(2 * M) * 0.1}
    p = {k: a.to("cuda").requires_grad_(True) for k, a in p0.items()}
    tail = lambda q, f: torch.tanh(f @ q["W2"].T + q["b2"]) @ q["W3"].T + q["b3"]        # noqa: E731

    def fn(q, o):
        return tail(q, pooled_features(env, o[0], o[1], q["W"], q["b"], "relu", 1.0, q["gamma"], q["beta"], forward_ad=True))

    def fn_torch(q, o):
        x, v = o
        ang = 2 * np.pi * x / L
        z = torch.stack([torch.cos(ang), torch.sin(ang), v], dim=-1) @ q["W"].T + q["b"]
        return tail(q, torch.relu(torch.nn.functional.layer_norm(z, (H,), q["gamma"], q["beta"], 1e-5)).mean(dim=-2))

    dps = [{k: r(*a.shape).to("cuda") for k, a in p0.items()} for _ in range(K)]
    del dps[1]["b"]
    w_hist, w_act = r(3, T, E).to("cuda"), r(T, E, 2 * M).to("cuda")
    ke, pe, per, acts, _ = grad.rollout_policy(env, lambda o: fn(p, o), T, observe="state", checkpoint_every=3)
    ((torch.stack([ke, pe, per]) * w_hist).sum() + (acts * w_act).sum()).backward()
    env.stop_tape()
    env.reset(X, V)
    pd = {k: a.detach() for k, a in p.items()}
    out = grad.rollout_policy_jvp(env, fn, pd, dps, T, observe="state", checkpoint_every=3)
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    worst = 0.0
    for k in range(K):
        lhs = float((torch.stack([out["dKE"][k], out["dPE"][k], out["dPE_reward"][k]]) * w_hist).sum() + (out["d_actions"][k] * w_act).sum())
        rhs = float(sum((p[name].grad * d).sum() for name, d in dps[k].items()))
        worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    record_measure("pool_jvp_closed_loop_duality", worst)
    env.reset(X, V)
    ref = grad.rollout_policy_jvp(env, fn_torch, pd, dps, T, observe="state", checkpoint_every=3)
    env.stop_tape()
    env.close()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())                        # noqa: E731
    err = max(rel(out[k], ref[k]) for k in ("dKE", "dPE", "dPE_reward", "d_actions", "d_x", "d_v"))
    record_measure("pool_jvp_closed_loop_vs_torch_layers", err)
    assert worst < DUALITY_BOUND, worst
    assert err < GRAD_BOUND, err
