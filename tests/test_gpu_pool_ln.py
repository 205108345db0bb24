"""Pooled particle features with a LayerNorm on the device (pic_pool_ln, pic_pool_ln_vjp, control/pool.py): parity
with the float64 restatement of tests/hp_pool_ln.py over the grid and with the reference encoder's recorded results (g19),
order-freeness and reproducibility bit for bit, the edges the contract defines, the refusals by message, and the closed loop
through rollout_policy(observe="state")."""
import itertools

import numpy as np
import pytest
import torch

import hp_pool as hp
import hp_pool_ln as hpl
from conftest import record_measure, rel_err
from test_gpu_pool import _bits, _cuda, _np, _same, _same_results  # noqa: F401

pytestmark = pytest.mark.gpu

L = hpl.L
ACTS = hpl.ACTS
KEYS = ("g_x", "g_v", "g_W", "g_b", "g_gamma", "g_beta")


def _env(E, N, Ng=64, L_=L, **kw):
    from ocplasma_amd.env.batched import BatchedPIC
    return BatchedPIC(E, N, Ng, L=L_, dt=0.1, **kw)


def _fwd(env, p, act, x=None, v=None, **kw):
    return env.pool(p[0], p[1], act, x=x, v=v, gamma=p[2], beta=p[3], **kw)


def _vjp(env, p, cot, act, x=None, v=None, **kw):
    return env.pool_vjp(p[0], p[1], cot, act, x=x, v=v, gamma=p[2], beta=p[3], **kw)


def _stack(sets, which):
    return tuple(np.stack([sets[s][i] for s in which]) for i in range(4))


# ---- 1. parity with the restatement -------------------------------------------------------------------------------------------------
def _vs_restatement(out, g, N, H, rows, which, act, per_env):
    """(forward, VJP) errors of a call on the grid's environments `rows` under the parameter sets `which` against the restatement,
    relative to each output's contract bound; shared parameters: against the sum of the environments' in ascending order."""
    X, V, sets, cot = hpl.grid_case(N, H)
    ef = eg = 0.0
    summed, scales = None, None
    for i, (e, s) in enumerate(zip(rows, which)):
        ref = hpl.restated(N, H, e, s, act)[0]
        got = (g["g_x"][i], g["g_v"][i]) + (tuple(g[k][i] for k in KEYS[2:]) if per_env else (None,) * 4)
        a, c = hpl.errors(out[i], got, ref, X[e], V[e], *sets[s], cot[e], L, act)
        ef, eg = max(ef, a), max(eg, c)
        if not per_env:
            sc = hpl.vjp_scales(X[e], V[e], sets[s][0], sets[s][1], sets[s][2], cot[e], L, 1.0, 1e-5)[2:]
            summed = list(ref[3:]) if summed is None else [a_ + b_ for a_, b_ in zip(summed, ref[3:])]
            scales = list(sc) if scales is None else [a_ + b_ for a_, b_ in zip(scales, sc)]
    if not per_env:
        for k, want, sc in zip(KEYS[2:], summed, (scales[0][:, None], scales[0], scales[1], scales[2])):
            eg = max(eg, float(np.max(np.abs(g[k] - want) / sc)))
    return ef, eg


@pytest.mark.parametrize("H", hpl.GRID_H)
@pytest.mark.parametrize("N", hpl.GRID_N)
def test_parity_with_the_restatement(N, H):
    """Forward and VJP against the float64 restatement for relu and tanh, shared and per-environment parameters, in a batch of
    three and alone.  The stored-particle, host-memory and device-memory forms are the same kernels on the same data and must
    agree with the checked result bit for bit."""
    X, V, sets, cot = hpl.grid_case(N, H)
    env3, env1 = _env(3, N), _env(1, N)
    worst = {"forward": 0.0, "vjp": 0.0}
    for env, E in ((env3, 3), (env1, 1)):
        env.reset(X[:E], V[:E])
        Xs, Vs = env.particles()                   # what the NULL form reads (the reset's stored particles)
        for act, per_env in itertools.product(ACTS, (False, True)):
            which = [1, 0, 0][:E] if per_env else [0] * E
            p = _stack(sets, which) if per_env else sets[0]
            x, v, c = X[:E], V[:E], cot[:E]
            out, g = _fwd(env, p, act, x, v), _vjp(env, p, c, act, x, v)
            ef, eg = _vs_restatement(out, g, N, H, range(E), which, act, per_env)
            worst["forward"], worst["vjp"] = max(worst["forward"], ef), max(worst["vjp"], eg)
            # the other forms of the same call
            tp, (tc, tx, tv) = _cuda(*p), _cuda(c, x, v)
            assert _same_results(out, g, _fwd(env, tp, act, tx, tv), _vjp(env, tp, tc, act, tx, tv)), (act, E, per_env, "device")
            so, sg = _fwd(env, p, act, Xs, Vs), _vjp(env, p, c, act, Xs, Vs)
            assert _same_results(so, sg, _fwd(env, p, act), _vjp(env, p, c, act)), (act, E, per_env, "stored, host")
            assert _same_results(so, sg, _fwd(env, tp, act), _vjp(env, tp, tc, act)), (act, E, per_env, "stored, device")
            if np.array_equal(Xs, x) and np.array_equal(Vs, v):
                assert _same_results(out, g, so, sg)
    record_measure(f"pool_ln_parity_forward_N{N}_H{H}", worst["forward"])
    record_measure(f"pool_ln_parity_vjp_N{N}_H{H}", worst["vjp"])
    print(f"pool_ln parity N={N} H={H}: forward {worst['forward']:.3e} (bound {hpl.bound('forward', N):.3e}) "
          f"vjp {worst['vjp']:.3e} (bound {hpl.bound('vjp', N):.3e})")
    assert worst["forward"] < hpl.bound("forward", N) and worst["vjp"] < hpl.bound("vjp", N), worst
    env3.close()
    env1.close()


# ---- 2. parity with the reference encoder (g19) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_env", [50.0, 37.0])
@pytest.mark.parametrize("pre", hpl.G19_CASES)
def test_parity_with_the_reference_encoder(pre, L_env):
    """PoolEncoder.from_reference and ReferenceEncoder on g19's cases (x_norm = 2, v_norm = 10 among them), on a handle with the
    encoder's period and on one with another L, which `period` must override.  Bound: the restatement's plus the restatement's own
    distance from g19."""
    from ocplasma_amd.control.pool import PoolEncoder, ReferenceEncoder
    g, sd, period, v_scale = hpl.g19_case(pre)
    E, N, H = g["x"].shape[0], int(g["N"]), int(g["H"])
    env = _env(E, N, L_=L_env)
    env.use_torch_stream()
    rf, rg = hpl.g19_restatement_error()
    bf, bg = hpl.bound("forward", N) + rf, hpl.bound("vjp", N) + rg
    x, v = (torch.tensor(g[k], device="cuda", requires_grad=True) for k in ("x", "v"))
    enc = PoolEncoder.from_reference(env, sd, float(hpl.G19["L"]), float(g["x_norm"]), float(g["v_norm"]))
    assert enc.period == period and enc.v_scale == v_scale and enc.eps == 1e-5 and enc.activation == "relu"
    out = enc((x, v))
    params = [enc.W, enc.b, enc.gamma, enc.beta]
    gr = torch.autograd.grad((out * torch.as_tensor(g["cot_phi"], device="cuda")).sum(), [x, v] + params)
    ef, eg = hpl.g19_errors(pre, _np(out), [_np(a) for a in gr])
    record_measure(f"pool_ln_g19_{pre}_L{L_env:g}_forward", ef)
    record_measure(f"pool_ln_g19_{pre}_L{L_env:g}_vjp", eg)
    assert ef < bf and eg < bg, (ef, bf, eg, bg)
    if H == 1:
        assert all(not _np(a).any() for a in gr[:4])                       # exact zeros, where autograd has roundoff / sqrt(eps)
    # the whole encoder: rho's float64 torch layers behind the op
    full = ReferenceEncoder(env, sd, float(hpl.G19["L"]), float(g["x_norm"]), float(g["v_norm"]))
    y = full((x, v))
    # what rho makes of the forward's bound: first order through its Jacobian at the recorded features, doubled, plus a float64
    # roundoff of rho's own (1e-14 of values of order 1, a hundred ulps)
    pooled = torch.tensor(g["phi_mean"], device="cuda")
    J = torch.autograd.functional.jacobian(full.rho, pooled).abs()      # [E, H_out, E, H]
    delta = torch.as_tensor(bf * hpl.forward_scale(sd[hpl.PHI[2]], sd[hpl.PHI[3]], "relu"), device="cuda")
    tol = 2.0 * torch.einsum("aobh,h->ao", J, delta) + 1e-14
    err = (y.detach() - torch.as_tensor(g["enc"], device="cuda")).abs()
    record_measure(f"pool_ln_g19_{pre}_L{L_env:g}_encoder_abs", float(err.max()))
    assert bool((err <= tol).all()), (err, tol)
    # its gradients with respect to x, v and phi's four tensors, for the cotangent rho hands down at the recorded features
    names = list(dict(full.named_parameters()))
    gy = torch.autograd.grad((y * torch.as_tensor(g["cot_enc"], device="cuda")).sum(), [x, v] + list(full.phi.parameters()))
    pooled.requires_grad_(True)
    cot_eff = torch.autograd.grad((full.rho(pooled) * torch.as_tensor(g["cot_enc"], device="cuda")).sum(), pooled)[0]
    _, eg2 = hpl.g19_errors(pre, None, [_np(a) for a in gy], _np(cot_eff), [g["genc_" + k] for k in ("x", "v") + hpl.PHI])
    record_measure(f"pool_ln_g19_{pre}_L{L_env:g}_encoder_vjp", eg2)
    assert len(names) == 8 and eg2 < 2 * bg, (eg2, bg)      # (twice: the cotangent itself carries the forward's difference)
    env.close()


# ---- 3. order-freeness, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
def test_results_do_not_depend_on_order_batch_geometry_or_run(act):
    E, N, H = 2, 4097, 5
    X, V = hp.box_data(E, N, seed=21)
    p = hpl.layer(H, seed=3)
    cot = np.random.default_rng(5).normal(0.0, 1.0, (E, H))
    env = _env(E, N)
    env.reset(X, V)
    Xs, Vs = env.particles()
    out, g = _fwd(env, p, act), _vjp(env, p, cot, act)
    assert _same_results(out, g, _fwd(env, p, act), _vjp(env, p, cot, act))                          # two runs
    perm = np.random.default_rng(6).permutation(N)
    Xp, Vp = Xs.copy(), Vs.copy()
    Xp[1], Vp[1] = Xs[1][perm], Vs[1][perm]
    outp, gp = _fwd(env, p, act, Xp, Vp), _vjp(env, p, cot, act, Xp, Vp)
    assert _same(out, outp) and all(_same(g[k], gp[k]) for k in KEYS[2:])
    assert _same(g["g_x"][1][perm], gp["g_x"][1]) and _same(g["g_v"][1][perm], gp["g_v"][1]) and _same(g["g_x"][0], gp["g_x"][0])
    env.close()
    for bpe in (1, 7):                                                                              # another launch geometry of the handle
        other = _env(E, N, blocks_per_env=bpe)
        other.reset(X, V)
        assert _same_results(out, g, _fwd(other, p, act), _vjp(other, p, cot, act)), bpe
        other.close()
    # environment 1 alone, and at row 299 of a batch of 300 (per-environment parameters: its own gradient)
    pe = tuple(np.broadcast_to(a, (300,) + a.shape).copy() for a in p)
    big = _env(300, N)
    Xb, Vb, cb = np.tile(Xs[0], (300, 1)), np.tile(Vs[0], (300, 1)), np.tile(cot[0], (300, 1))
    Xb[299], Vb[299], cb[299] = Xs[1], Vs[1], cot[1]
    ob, gb = _fwd(big, pe, act, Xb, Vb), _vjp(big, pe, cb, act, Xb, Vb)
    big.close()
    one = _env(1, N)
    p1 = tuple(a[None] for a in p)
    o1, g1 = _fwd(one, p1, act, Xs[1:], Vs[1:]), _vjp(one, p1, cot[1:], act, Xs[1:], Vs[1:])
    one.close()
    assert _same(o1[0], ob[299]) and _same(o1[0], out[1])
    assert all(_same(g1[k][0], gb[k][299]) for k in KEYS)
    assert _same(g1["g_x"][0], g["g_x"][1]) and _same(g1["g_v"][0], g["g_v"][1])


def test_two_chunks_per_workgroup_match_a_one_environment_handle():
    """4096 x 1025 at H = 3: the shape hp_pool.plan pins at two chunks per workgroup, against a handle of one environment (one
    chunk per workgroup, two workgroups)."""
    E, N, H = 4096, 1025, 3
    assert hp.plan(E, N)["chunks_per_wg"] == 2 and hp.plan(1, N) == {"nchunks": 2, "wpe": 2, "chunks_per_wg": 1, "workgroups": 2}
    X, V = hp.box_data(2, N, seed=33)
    p = hpl.layer(H, seed=8)
    cot = np.random.default_rng(9).normal(0.0, 1.0, (2, H))
    pe = tuple(np.broadcast_to(a, (E,) + a.shape).copy() for a in p)
    Xb, Vb, cb = np.tile(X[0], (E, 1)), np.tile(V[0], (E, 1)), np.tile(cot[0], (E, 1))
    Xb[E - 1], Vb[E - 1], cb[E - 1] = X[1], V[1], cot[1]
    big, one = _env(E, N), _env(1, N)
    p1 = tuple(a[None] for a in p)
    for act in ACTS:
        ob, gb = _fwd(big, pe, act, Xb, Vb), _vjp(big, pe, cb, act, Xb, Vb)
        for row, e in ((0, 0), (E - 1, 1)):
            o1, g1 = _fwd(one, p1, act, X[e:e + 1], V[e:e + 1]), _vjp(one, p1, cot[e:e + 1], act, X[e:e + 1], V[e:e + 1])
            assert _same(o1[0], ob[row]) and all(_same(g1[k][0], gb[k][row]) for k in KEYS), (act, row)
    big.close()
    one.close()


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------
def _edge_case(E=3, N=1000, H=5, seed=41, lead=False):
    X, V = hp.box_data(E, N, seed=seed)
    p = hpl.layer(H, seed=seed + 1, lead=(E,) if lead else ())
    return X, V, p, np.random.default_rng(seed + 2).normal(0.0, 1.0, (E, H))


def _restated_batch(X, V, p, cot, act, period=L, eps=1e-5):
    """The restatement over a batch with per-environment parameters: (out [E, H], the six gradients stacked)."""
    rows = [(hpl.forward(X[e], V[e], *(a[e] for a in p), period, act, eps=eps),
             hpl.vjp(X[e], V[e], *(a[e] for a in p), cot[e], period, act, eps=eps)) for e in range(len(X))]
    return np.stack([r[0] for r in rows]), [np.stack([r[1][i] for r in rows]) for i in range(6)]


def _batch_errors(out, g, X, V, p, cot, act, period=L, eps=1e-5):
    ro, rg = _restated_batch(X, V, p, cot, act, period, eps)
    ef = eg = 0.0
    for e in range(len(X)):
        pe = tuple(a[e] for a in p)
        a, c = hpl.errors(out[e], tuple(g[k][e] for k in KEYS), (ro[e],) + tuple(r[e] for r in rg), X[e], V[e], *pe, cot[e], period,
                          act, eps=eps)
        ef, eg = max(ef, a), max(eg, c)
    return ef, eg


@pytest.mark.parametrize("act", ACTS)
def test_equal_rows_eps_one_and_positions_off_the_box(act):
    """All rows of W (and b) equal: var = 0, r = 1 / sqrt(eps), out = act(beta).  eps = 1.  Positions at -0.0, the last double
    below L and 3.3 L.  Each against the restatement under the grid's bound."""
    E, N, H = 2, 1000, 5
    X, V, p, cot = _edge_case(E, N, H, lead=True)
    X[:, 0], X[:, 1], X[:, 2] = -0.0, np.nextafter(L, 0.0), 3.3 * L
    env = _env(E, N)
    for name, pp, eps in (("off the box", p, 1e-5), ("eps = 1", p, 1.0),
                          ("equal rows", (np.broadcast_to(p[0][:, :1], p[0].shape).copy(), np.broadcast_to(p[1][:, :1], p[1].shape).copy(), p[2], p[3]), 1e-5)):
        out, g = _fwd(env, pp, act, X, V, eps=eps), _vjp(env, pp, cot, act, X, V, eps=eps)
        ef, eg = _batch_errors(out, g, X, V, pp, cot, act, eps=eps)
        record_measure(f"pool_ln_edge_{name.replace(' ', '_')}_{act}", max(ef, eg))
        if name == "equal rows":
            # d is the rounding of the mean alone, at most H ulps of |z| < 32, and so is its difference between two libms:
            # |y| < 5 * 32 * 2^-52 / sqrt(eps) = 1.2e-11.  It enters n times |gamma| < 1.5 (the activations have slope <= 1) and
            # dz through y m2 and m2 = mean(dy y), each at most |y| of dz's bound: 4e-11 on top of the grid's bound
            want = np.tanh(pp[3]) if act == "tanh" else np.maximum(pp[3], 0.0)
            assert np.max(np.abs(out - want)) < 1e-10
            assert ef < hpl.bound("forward", N) + 4e-11 and eg < hpl.bound("vjp", N) + 4e-11, (name, ef, eg)
        else:
            assert ef < hpl.bound("forward", N) and eg < hpl.bound("vjp", N), (name, ef, eg)
    env.close()


@pytest.mark.parametrize("act", ACTS)
def test_zero_gamma_period_and_cotangent_scales(act):
    E, N, H = 3, 1000, 5
    X, V, p, cot = _edge_case(E, N, H, lead=True)
    env = _env(E, N)
    g = _vjp(env, p, cot, act, X, V)
    # gamma_k = 0 (and beta_k = 0 for relu): a zero bound deposits nothing, +0
    pz = tuple(a.copy() for a in p)
    pz[2][:, 2] = 0.0
    pz[3][:, 2] = 0.0
    oz, gz = _fwd(env, pz, act, X, V), _vjp(env, pz, cot, act, X, V)
    assert _same(oz[:, 2], np.zeros(E))
    if act == "relu":                                       # (n = 0 is not > 0: a = 0, every term of g_gamma_k and g_beta_k is 0)
        assert _same(gz["g_gamma"][:, 2], np.zeros(E)) and _same(gz["g_beta"][:, 2], np.zeros(E))
    assert np.isfinite(oz).all() and all(np.isfinite(gz[k]).all() for k in KEYS)
    # period 0 is the handle's L, bit for bit; another period is another function
    o0, g0 = _fwd(env, p, act, X, V, period=0.0), _vjp(env, p, cot, act, X, V, period=0.0)
    assert _same_results(o0, g0, _fwd(env, p, act, X, V, period=L), _vjp(env, p, cot, act, X, V, period=L))
    assert _same_results(o0, g0, _fwd(env, p, act, X, V), g)
    assert not _same(o0, _fwd(env, p, act, X, V, period=2 * L))
    # the cotangent of an environment scaled by 2^100, 2^-100 and 0
    scale = np.array([2.0 ** 100, 2.0 ** -100, 0.0])
    gs = _vjp(env, p, cot * scale[:, None], act, X, V)
    for k in KEYS:
        for e in range(E):
            assert _same(g[k][e] * scale[e] + 0.0, gs[k][e]), (k, e)
        assert not np.signbit(gs[k][2]).any(), k
    env.close()


def test_huge_and_non_finite_input_poisons_its_environment_alone():
    E, N, H = 3, 1000, 5
    X, V, p, cot = _edge_case(E, N, H, lead=True)
    env = _env(E, N)
    for act in ACTS:
        clean, gc = _fwd(env, p, act, X, V), _vjp(env, p, cot, act, X, V)

        def only_env_1_is_nan(out, g, what):
            if out is not None:
                assert np.isnan(out[1]).all(), (act, what)
                assert _same(out[[0, 2]], clean[[0, 2]]), (act, what)
            if g is not None:
                assert all(np.isnan(g[k][1]).all() for k in KEYS), (act, what)
                assert all(_same(g[k][[0, 2]], gc[k][[0, 2]]) for k in KEYS), (act, what)
            # ... and the next call finds the work block clean
            assert _same_results(clean, gc, _fwd(env, p, act, X, V), _vjp(env, p, cot, act, X, V)), (act, what)

        # v = 1e300: finite z and var (|W_k2| u_max < 2^500 fails: 1e300 > 2^500 = 3e150, so the rule makes the environment NaN)
        Vh = V.copy()
        Vh[1, 17] = 1e300
        only_env_1_is_nan(_fwd(env, p, act, X, Vh), _vjp(env, p, cot, act, X, Vh), "v = 1e300")
        # v = 1e100 is below the rule's 2^500: finite results
        Vh[1, 17] = 1e100
        out, g = _fwd(env, p, act, X, Vh), _vjp(env, p, cot, act, X, Vh)
        assert np.isfinite(out).all() and all(np.isfinite(g[k]).all() for k in KEYS), act
        Vi = V.copy()
        Vi[1, 17] = np.inf
        only_env_1_is_nan(_fwd(env, p, act, X, Vi), _vjp(env, p, cot, act, X, Vi), "v = inf")
        Xn = X.copy()
        Xn[1, N - 1] = np.nan
        only_env_1_is_nan(_fwd(env, p, act, Xn, V), _vjp(env, p, cot, act, Xn, V), "x = nan")
        # a NaN in one W_k. poisons the environment in both calls (the mean over k)
        pw = tuple(a.copy() for a in p)
        pw[0][1, 3, 1] = np.nan
        only_env_1_is_nan(_fwd(env, pw, act, X, V), _vjp(env, pw, cot, act, X, V), "W nan")
        # a NaN in one gamma_k: out_k alone in the forward, the environment in the VJP
        pg = tuple(a.copy() for a in p)
        pg[2][1, 3] = np.nan
        out = _fwd(env, pg, act, X, V)
        rest = [0, 1, 2, 4]
        assert np.isnan(out[1, 3]) and _same(out[1, rest], clean[1, rest]) and _same(out[[0, 2]], clean[[0, 2]]), act
        only_env_1_is_nan(None, _vjp(env, pg, cot, act, X, V), "gamma nan")
        # a NaN in one cot_k: the environment
        cn = cot.copy()
        cn[1, 0] = np.nan
        only_env_1_is_nan(None, _vjp(env, p, cn, act, X, V), "cot nan")
    env.close()


def test_every_subset_of_outputs_and_the_ops_routing():
    from ocplasma_amd.control.pool import pooled_features
    E, N, H = 2, 1025, 5
    X, V, p, cot = _edge_case(E, N, H)
    env = _env(E, N)
    env.use_torch_stream()
    full = _vjp(env, p, cot, "relu", X, V)
    for gx, gv, gp in itertools.product((False, True), repeat=3):
        g = _vjp(env, p, cot, "relu", X, V, g_x=gx, g_v=gv, g_params=gp)
        for k, on in zip(KEYS, (gx, gv, gp, gp, gp, gp)):
            assert (g[k] is None) if not on else _same(g[k], full[k]), (gx, gv, gp, k)
    # the op computes what needs_input_grad asks for, and the same bits
    names = ("x", "v", "W", "b", "gamma", "beta")
    for need in itertools.product((False, True), repeat=6):
        if not any(need):
            continue
        t = [torch.tensor(a, device="cuda", requires_grad=n) for a, n in zip((X, V) + tuple(p), need)]
        out = pooled_features(env, t[0], t[1], t[2], t[3], "relu", 1.0, t[4], t[5])
        out.backward(torch.as_tensor(cot, device="cuda"))
        for name, k, ti, n in zip(names, KEYS, t, need):
            assert (ti.grad is None) if not n else _same(ti.grad, full[k]), (need, name)
    env.close()


def test_alternating_plain_and_layernorm_calls_share_the_block():
    """One handle through pic_pool and pic_pool_ln calls of changing H (they share the work block and its zero head) against fresh
    handles."""
    E, N = 2, 1025
    X, V = hp.box_data(E, N, seed=71)
    env = _env(E, N)
    calls = [("ln", 5), ("plain", 64), ("ln", 64), ("plain", 3), ("ln", 256), ("ln", 1), ("plain", 256), ("ln", 5)]
    for i, (kind, H) in enumerate(calls):
        p = hpl.layer(H, seed=i)
        cot = np.random.default_rng(i).normal(0.0, 1.0, (E, H))
        fresh = _env(E, N)
        for e_ in (env, fresh):
            if kind == "ln":
                res = (_fwd(e_, p, "relu", X, V), _vjp(e_, p, cot, "relu", X, V))
            else:
                res = (e_.pool(p[0], p[1], "relu", x=X, v=V), e_.pool_vjp(p[0], p[1], cot, "relu", x=X, v=V))
            if e_ is env:
                mine = res
        fresh.close()
        assert _same(mine[0], res[0]) and all(_same(mine[1][k], res[1][k]) for k in res[1]), (i, kind, H)
    env.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    from ocplasma_amd import _abi
    E, N, H = 2, 100, 4
    env = _env(E, N)
    X, V = hp.box_data(E, N, seed=51)
    p = np.zeros(6 * H)
    out, cot, gx = np.zeros((E, H)), np.ones((E, H)), np.zeros((E, N))
    A = lambda a: a.ctypes.data

    def spec(hidden=H, activation=0, per_env=0, params_kind=_abi.PIC_HOST, v_scale=1.0, eps=1e-5, period=0.0, params=A(p)):
        return _abi.PicPoolLnSpec(hidden, activation, per_env, params_kind, v_scale, eps, period, params)

    def both(why, s, x=A(X), v=A(V), kind=_abi.PIC_HOST):
        with pytest.raises(_abi.PicError, match=why):
            env._h.pool_ln(s, x, v, kind, A(out))
        with pytest.raises(_abi.PicError, match=why):
            env._h.pool_ln_vjp(s, x, v, A(cot), kind, A(gx), 0, 0)
    for eps in (0.0, -1e-5, float("inf"), float("nan")):
        both(r"error -1: pic_pool_ln\w*: eps must be finite and > 0", spec(eps=eps))
    for period in (-1.0, float("inf"), float("nan")):
        both(r"error -1: pic_pool_ln\w*: period must be finite and >= 0", spec(period=period))
    both(r"error -1: pic_pool_ln\w*: hidden must be 1\.\.256", spec(hidden=0))
    both(r"error -1: pic_pool_ln\w*: hidden must be 1\.\.256", spec(hidden=257))
    both(r"error -1: pic_pool_ln\w*: activation must be", spec(activation=2))
    both(r"error -1: pic_pool_ln\w*: per_env must be 0 or 1", spec(per_env=2))
    both(r"error -1: pic_pool_ln\w*: bad params_mem_kind", spec(params_kind=7))
    both(r"error -1: pic_pool_ln\w*: params is NULL", spec(params=None))
    both(r"error -1: pic_pool_ln\w*: v_scale is not finite", spec(v_scale=float("nan")))
    both(r"error -1: pic_pool_ln\w*: bad mem_kind", spec(), kind=5)
    both(r"error -1: pic_pool_ln\w*: x and v must both be given or both be NULL", spec(), v=0)
    both(r"error -1: pic_pool_ln\w*: x and v must both be given or both be NULL", spec(), x=0)
    with pytest.raises(_abi.PicError, match="error -1: pic_pool_ln: out is NULL"):
        env._h.pool_ln(spec(), A(X), A(V), _abi.PIC_HOST, 0)
    with pytest.raises(_abi.PicError, match="error -1: pic_pool_ln_vjp: cot is NULL"):
        env._h.pool_ln_vjp(spec(), A(X), A(V), 0, _abi.PIC_HOST, A(gx), 0, 0)
    # the stored particles: PIC_ESTATE before pic_reset, PIC_EINVAL on a float32 handle
    both(r"error -3: pic_pool_ln\w*: call pic_reset first", spec(), x=0, v=0)
    env.reset(X, V)
    env._h.pool_ln(spec(), 0, 0, _abi.PIC_HOST, A(out))
    env.close()
    env = _env(E, N, dtype="float32")
    env.reset(X, V)
    both(r"error -1: pic_pool_ln\w*: the stored particles need float64 particles with float64 positions", spec(), x=0, v=0)
    env._h.pool_ln(spec(), A(X), A(V), _abi.PIC_HOST, A(out))          # (given particles need no float64 state)
    env.close()


# ---- 6. the closed loop -----------------------------------------------------------------------------------------------------------------
def test_closed_loop_matches_the_same_policy_in_torch_layers():
    """rollout_policy(observe="state") under head(rho(PoolEncoder(layernorm=True)(x, v))) against the same policy written with torch
    layers (nn.Linear(3, H), nn.LayerNorm, the mean) through the same call: traces and parameter gradients within
    test_gpu_policy_grad's bound."""
    from ocplasma_amd.control.pool import PoolEncoder
    from ocplasma_amd.env import grad
    from test_gpu_policy_grad import GRAD_BOUND, M, _make, _weights
    E, N, Ng, T, H, Ho = 2, 257, 32, 3, 8, 6
    env, X, V = _make(E, N, Ng, seed=7)
    env.use_torch_stream()
    gen = torch.Generator().manual_seed(5)
    enc = PoolEncoder(env, H, "relu", layernorm=True, generator=gen)
    with torch.no_grad():
        enc.gamma.copy_(torch.empty(H, dtype=torch.float64).uniform_(-1.5, 1.5, generator=gen))
        enc.beta.copy_(torch.empty(H, dtype=torch.float64).uniform_(-1.0, 1.0, generator=gen))
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(H, Ho, dtype=torch.float64), torch.nn.LayerNorm(Ho, dtype=torch.float64),
                                     torch.nn.ReLU(), torch.nn.Linear(Ho, 2 * M, dtype=torch.float64)).to("cuda")
    torch.manual_seed(6)
    tail_a, tail_b = mk(), mk()
    tail_b.load_state_dict(tail_a.state_dict())
    lin, norm = torch.nn.Linear(3, H, dtype=torch.float64).to("cuda"), torch.nn.LayerNorm(H, dtype=torch.float64).to("cuda")
    with torch.no_grad():
        lin.weight.copy_(enc.W)
        lin.bias.copy_(enc.b)
        norm.weight.copy_(enc.gamma)
        norm.bias.copy_(enc.beta)

    def torch_policy(xv):
        x, v = xv
        q = 2 * np.pi * x / L
        f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1)
        return tail_b(torch.relu(norm(lin(f))).mean(dim=-2))

    wh = torch.as_tensor(_weights(T, E, M, seed=4)[0], device="cuda")

    def loss(policy):
        ke, pe, per, acts, obs = grad.rollout_policy(env, policy, T, observe="state")
        hist = torch.stack([ke, pe, per], -1)
        return (hist * wh).sum() + 0.05 * (acts ** 2).sum(), hist

    J, hist = loss(lambda o: tail_a(enc(o)))
    J.backward()
    got = [t.grad.cpu().numpy().ravel() for t in (enc.W, enc.b, enc.gamma, enc.beta, *tail_a.parameters())]
    env.stop_tape()
    env.reset(X, V)
    Jt, hist_t = loss(torch_policy)
    Jt.backward()
    want = [t.grad.cpu().numpy().ravel() for t in (lin.weight, lin.bias, norm.weight, norm.bias, *tail_b.parameters())]
    env.stop_tape()
    env.close()
    err = rel_err(np.concatenate(got), np.concatenate(want))
    err_hist = rel_err(hist.detach().cpu().numpy(), hist_t.detach().cpu().numpy())
    record_measure("pool_ln_closed_loop_grad_rel_err", err)
    record_measure("pool_ln_closed_loop_trace_rel_err", err_hist)
    assert err < GRAD_BOUND and err_hist < GRAD_BOUND, (err, err_hist)
