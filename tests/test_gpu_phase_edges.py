"""The smoothed phase-space density, its KL, the gradient gather and the forward-mode product on the device (pic_phase_kl_smooth*,
DESIGN.md 7g, 7j) at the edges of phase_locate and of the banded deposit: the constructed states and the np.longdouble reference
of tests/hp_phase_cases.py, through the public methods of BatchedPIC with no step.  Every case is loaded twice
(hp_phase_cases.LOADS): by reset(X, V), whose refresh stores the folded positions (asserted here against the host's fold), so that
x = L, a position outside the box or a non-finite one never reaches phase_locate; and by the handle's set_particles, which keeps
them and is the only way to the inclusive `x <= L`, the drop by x and a NaN position.  The premises (every edge class present,
the reference against automatic differentiation, the floors) are pinned by tests/test_phase_edges_cpu.py.

Bounds (hp_phase_cases.bound): the density bitwise; KL within max(3.4e-14, 100 x floor) of the condition scale S_kl; the gradient
within max(5.4e-14, 100 x floor) of the largest reference entry; the forward mode within 100 x gradient floor + N 2^-52 of
S_jvp; none above 1e-9; and exactly 0 wherever the reference is exactly 0.  The floor is the float64 restatement (hp_phase.py)
against the longdouble reference at that case.  Every measured error, floor and bound is recorded under
phase_edges.<case>.<load>.<surface> and listed in profiles/phase_edges.md.

Device results are computed once per case and load, every call made twice in a row on the same handle (the finishing kernel clears the
integer sums behind itself), and shared by the tests; nothing modifies them."""
import functools

import numpy as np
import pytest
import torch

import hp_phase as hp
import hp_phase_cases as pc
from conftest import record_measure

pytestmark = pytest.mark.gpu

ALL = [(cid, load) for cid in pc.CASES for load in pc.LOADS]
IDS = [f"{cid}-{load}" for cid, load in ALL]
NG = 8                        # the field mesh plays no part here
WHICH = ("x", "v", "both")
DEVICE_INPUT_CASES = ("E", "G")


def _make(cid, load):
    """A handle of the case's state, loaded by reset (the refresh folds x) or by set_particles (x as given): the particles it
    then holds are hp_phase_cases.particles(cid, load), the ones the reference is evaluated on."""
    from ocplasma_amd.env.batched import BatchedPIC
    c = pc.CASES[cid]
    X, V = pc.state(cid)
    env = BatchedPIC(c.E, c.N, NG, n0=c.n0, L=c.L, dt=0.01)
    assert env.n0 == c.n0 and env.L == c.L
    if load == "reset":
        env.reset(X, V)
    else:
        env._h.set_particles(X, V)
    x, v = env.particles()
    wx, wv = pc.particles(cid, load)
    bad = np.argwhere(~((x == wx) | (np.isnan(x) & np.isnan(wx))))
    assert bad.size == 0, (cid, load, len(bad), [(X[tuple(i)], x[tuple(i)], wx[tuple(i)]) for i in bad[:8]])
    assert np.array_equal(v, wv, equal_nan=True)
    return env


def _pick(tx, tv, which):
    return dict(d_x=tx if which != "v" else None, d_v=tv if which != "x" else None)


def _np(a):
    if isinstance(a, tuple):
        return tuple(_np(b) for b in a)
    return a.cpu().numpy() if torch.is_tensor(a) else a


@functools.lru_cache(maxsize=None)
def _device(cid, load):
    """name -> (first result, result of the same call made again at once) of every surface of the case loaded by `load`."""
    c = pc.CASES[cid]
    shared, per = pc.targets(cid)
    d = np.asarray(c.d_kl)
    vr = (c.vmin, c.vmax)
    env = _make(cid, load)
    out = {}

    def twice(name, fn):
        out[name] = (_np(fn()), _np(fn()))
    twice("f", lambda: env.phase_density_smooth((c.nx, c.nv), *vr))
    for name, feq in (("shared", shared), ("env", per)):
        twice(f"kl.{name}", lambda: env.kl_smooth(feq, *vr))
        twice(f"grad.{name}", lambda: env.kl_smooth_grad(feq, d, *vr))
    for K in pc.ks(cid):
        tx, tv = pc.tangents(cid, K)
        for which in WHICH:
            twice(f"jvp.{K}.{which}", lambda: env.kl_smooth_jvp(per, *vr, **_pick(tx, tv, which)))
        for k in range(K):
            twice(f"jvp.{K}.single{k}", lambda: env.kl_smooth_jvp(per, *vr, d_x=tx[k], d_v=tv[k]))
    if cid in DEVICE_INPUT_CASES:
        def cu(a):
            return torch.as_tensor(np.array(a), device="cuda")
        tx, tv = pc.tangents(cid, 3)
        twice("cuda.kl", lambda: env.kl_smooth(cu(per), *vr))
        twice("cuda.grad", lambda: env.kl_smooth_grad(cu(per), cu(d), *vr))
        twice("cuda.jvp", lambda: env.kl_smooth_jvp(cu(per), *vr, d_x=cu(tx), d_v=cu(tv)))
        assert all(torch.is_tensor(a) and a.is_cuda for a in (env.kl_smooth(cu(per), *vr), *env.kl_smooth_grad(cu(per), cu(d), *vr)))
    env.close()
    return out


def _check(cid, load, surface, err, kind):
    b, fl = pc.bound(cid, load, kind), pc.floors(cid, load)["kl" if kind == "kl" else "grad"]
    name = f"phase_edges.{cid}.{load}.{surface}"
    print(f"{name}: device {err:.3e}  floor {fl:.3e}  bound {b:.3e}")
    record_measure(name, err)
    record_measure(f"phase_edges.{cid}.{load}.floor.{'kl' if kind == 'kl' else 'grad'}", fl)
    record_measure(name + ".bound", b)
    assert err <= b, (name, err, b)


def _same(a, b):
    if isinstance(a, tuple):
        return all(_same(p, q) for p, q in zip(a, b))
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ---- 1. the density --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,load", ALL, ids=IDS)
def test_density_is_bitwise_the_restatement(cid, load):
    f = _device(cid, load)["f"][0]
    want = pc.ref(cid, load)["f"]
    record_measure(f"phase_edges.{cid}.{load}.f", float(np.abs(f - want).max()))
    bad = np.argwhere(f != want)
    assert bad.size == 0, (cid, len(bad), bad[:8], f[tuple(bad[0])], want[tuple(bad[0])])
    assert not np.signbit(f).any()


# ---- 2. the KL -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,load", ALL, ids=IDS)
def test_kl_matches_longdouble(cid, load):
    r, dev = pc.ref(cid, load), _device(cid, load)
    for name in ("shared", "env"):
        kl, want, S = dev[f"kl.{name}"][0], r[name]["kl"], r[name]["S_kl"]
        assert np.isfinite(kl).all()
        _check(cid, load, f"kl.{name}", pc.kl_err(kl, want, S), "kl")
        assert not kl[S == 0].any()


# ---- 3. the gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,load", ALL, ids=IDS)
def test_gradient_matches_longdouble_with_exact_zeros(cid, load):
    c, r, dev = pc.CASES[cid], pc.ref(cid, load), _device(cid, load)
    inside, _, _, _, _, _, _, slope = (a.numpy() for a in hp.locate(*(pc._t(a) for a in pc.particles(cid, load)), c.grid()))
    for name in ("shared", "env"):
        (gx, gv), (wx, wv) = dev[f"grad.{name}"][0], r[name]["grad"]
        assert gx.shape == gv.shape == (c.E, c.N) and np.isfinite(gx).all() and np.isfinite(gv).all()
        _check(cid, load, f"grad.{name}", pc.grad_err(gx, gv, (wx, wv)), "grad")
        # exactly 0 where the reference is: dropped and non-finite particles, g_v of clamped ones, nx = 1, nv = 1, d_kl = 0
        assert not gx[wx == 0].any() and not gv[wv == 0].any(), (cid, name)
        assert not gx[~inside].any() and not gv[~(inside & slope)].any(), (cid, name)
        assert not gx[np.asarray(c.d_kl) == 0].any() and not gv[np.asarray(c.d_kl) == 0].any()
    if cid == "B":
        assert not dev["grad.env"][0][0].any()
    if cid == "C":
        assert not dev["grad.env"][0][1].any()


# ---- 4. the forward mode ---------------------------------------------------------------------------------------------------------
JVP = [(cid, load, K) for cid, load in ALL for K in pc.ks(cid)]
JVP_IDS = [f"{cid}-{load}-K{K}" for cid, load, K in JVP]


@pytest.mark.parametrize("cid,load,K", JVP, ids=JVP_IDS)
def test_forward_mode_matches_longdouble(cid, load, K):
    c, dev = pc.CASES[cid], _device(cid, load)
    for which in WHICH:
        got = dev[f"jvp.{K}.{which}"][0]
        want, S = pc.ref_jvp(cid, load, K, which)
        assert got.shape == (K, c.E) and np.isfinite(got).all()
        ok = S > 0
        err = float((np.abs(got.astype(pc.LD) - want)[ok] / S[ok]).max()) if ok.any() else 0.0
        _check(cid, load, f"jvp.K{K}.{which}", err, "jvp")
        assert not got[~ok].any(), (cid, load, K, which)


@pytest.mark.parametrize("cid,load,K", JVP, ids=JVP_IDS)
def test_forward_mode_directions_in_one_call_are_the_single_calls(cid, load, K):
    dev = _device(cid, load)
    both = dev[f"jvp.{K}.both"][0]
    for k in range(K):
        single = dev[f"jvp.{K}.single{k}"][0]
        assert single.shape == both[k].shape and _same(single, both[k]), (cid, load, K, k, single, both[k])


# ---- 5. case I: a copied and an empty environment --------------------------------------------------------------------------------
@pytest.mark.parametrize("load", pc.LOADS)
def test_copied_environment_gives_the_same_bits_and_an_empty_one_plus_zero(load):
    dev = _device("I", load)
    for name, (a, _) in dev.items():
        if name.startswith("jvp"):
            if "single" in name:
                continue                                # (environment 2's tangents are its own)
            assert (a[:, 1] == 0).all() and not np.signbit(a[:, 1]).any(), name
        elif name.startswith("grad"):
            for g in a:
                assert (g[1] == 0).all() and not np.signbit(g[1]).any(), name
        else:
            assert (a[1] == 0).all() and not np.signbit(a[1]).any(), name
    assert _same(dev["f"][0][2], dev["f"][0][0])
    assert _same(dev["kl.shared"][0][2], dev["kl.shared"][0][0])
    # the same particles, target, cotangent and tangents in environments 0 and 2 of a handle of their own: the same bits
    c = pc.CASES["I"]
    per, d = pc.targets("I")[1].copy(), np.array([0.7, -1.3, 0.7])
    per[2] = per[0]
    tx, tv = (np.array(t) for t in pc.tangents("I", 3))
    tx[:, 2], tv[:, 2] = tx[:, 0], tv[:, 0]
    env = _make("I", load)
    kl = env.kl_smooth(per, c.vmin, c.vmax)
    gx, gv = env.kl_smooth_grad(per, d, c.vmin, c.vmax)
    jv = env.kl_smooth_jvp(per, c.vmin, c.vmax, d_x=tx, d_v=tv)
    env.close()
    assert _same(kl[2], kl[0]) and _same(gx[2], gx[0]) and _same(gv[2], gv[0]) and _same(jv[:, 2], jv[:, 0])
    assert gx[0].any() and gv[0].any() and jv[:, 0].all()
    assert _same(kl[0], dev["kl.env"][0][0]) and _same(gx[0], dev["grad.env"][0][0][0]) and _same(jv[:, 0], dev["jvp.3.both"][0][:, 0])


# ---- 6. device inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,load", [a for a in ALL if a[0] in DEVICE_INPUT_CASES], ids=[i for i in IDS if i[0] in DEVICE_INPUT_CASES])
def test_device_inputs_give_the_bits_of_the_host_path(cid, load):
    dev = _device(cid, load)
    assert _same(dev["cuda.kl"][0], dev["kl.env"][0])
    assert _same(dev["cuda.grad"][0], dev["grad.env"][0])
    assert _same(dev["cuda.jvp"][0], dev["jvp.3.both"][0])


# ---- 7. a second call on the same handle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,load", ALL, ids=IDS)
def test_second_call_returns_the_same_bits(cid, load):
    for name, (a, b) in _device(cid, load).items():
        assert _same(a, b), (cid, load, name)


# ---- 8. clamped half-bins have no v-slope, whatever the grid holds -----------------------------------------------------------------
@pytest.mark.parametrize("load", pc.LOADS)
def test_clamped_half_bins_have_no_v_slope_under_a_non_finite_grid(load):
    """A target of +inf in the two edge columns of v makes the cotangent grid there -inf (log 0): a clamped particle reads the
    same bin twice, and g_v must be the 0 of "no slope", not the NaN of inf - inf (hp_phase.vjp: where(inside & slope, ., 0))."""
    cid = "D1"
    c = pc.CASES[cid]
    X, V = pc.particles(cid, load)
    feq = pc.targets(cid)[0].copy()
    feq[:, 0] = feq[:, -1] = np.inf
    env = _make(cid, load)
    gx, gv = env.kl_smooth_grad(feq, np.asarray(c.d_kl), c.vmin, c.vmax)
    gx2, gv2 = env.kl_smooth_grad(feq, np.asarray(c.d_kl), c.vmin, c.vmax)
    env.close()
    inside, _, _, j0, j1, _, _, slope = (a.numpy() for a in hp.locate(pc._t(X), pc._t(V), c.grid()))
    clamped = inside & ~slope
    assert clamped[0].sum() >= 40 and ((j0 == 0) & clamped).any() and ((j1 == c.nv - 1) & clamped).any()
    assert not gv[clamped].any() and not gv[~inside].any() and not gx[~inside].any()
    wx, wv = (a.numpy() for a in hp.vjp(pc._t(X), pc._t(V), pc._t(feq), pc._t(c.d_kl), c.grid()))
    assert not wv[clamped].any()
    inner = inside & slope & (j0 > 0) & (j1 < c.nv - 1)              # particles that read no edge column: finite and as before
    assert np.isfinite(gx[inner]).all() and np.isfinite(gv[inner]).all()
    assert np.abs(gv[inner] - wv[inner]).max() <= pc.TOL_GRAD * np.abs(wv[inner]).max()
    assert np.array_equal(gx, gx2, equal_nan=True) and np.array_equal(gv, gv2, equal_nan=True)
