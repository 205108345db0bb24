"""The premises of tests/test_gpu_phase_edges.py, pinned without a GPU (tests/hp_phase_cases.py): every edge class the states are
built for is really there, the reference's mass is exact, the longdouble reference agrees with automatic differentiation where
that can be evaluated (the finite sub-state), the floors are small, and the band height is the host's.  Everything holds for
the particles as the kernels read them after either way of loading them (hp_phase_cases.LOADS)."""
import numpy as np
import pytest

import hp_phase as hp
import hp_phase_cases as pc

ALL = list(pc.CASES)
BIG = [cid for cid, c in pc.CASES.items() if c.N >= 255]
# the classes the first N pairs of a small case admit: (+0.0, vmin), (+0.0, vmax), (-0.0, vmin)
SMALL = {"A": ("wrap", "low"), "B": ("wrap", "low", "high"), "C": ("wrap", "low", "high")}


def _classes(cid, load, e=0):
    c = pc.CASES[cid]
    X, V = pc.particles(cid, load)
    x, v = X[e], V[e]
    G = c.grid()
    inside, i0, i1, j0, j1, fx, fv, slope = (a.numpy() for a in hp.locate(pc._t(x), pc._t(v), G))
    fin = np.isfinite(x) & np.isfinite(v)
    w = (v - c.vmin) * G.rdv - 0.5
    out = {"inside": inside, "slope": inside & slope,
           "drop_x": fin & ~((x >= 0) & (x <= c.L)), "drop_v": fin & ~((v >= c.vmin) & (v <= c.vmax)), "nonfinite": ~fin,
           "low": inside & ~slope & (w < 0), "high": inside & ~slope & ~(w < 0),
           "wrap": inside & (i0 == c.nx - 1) & (i1 == 0), "x_is_L": inside & (x == c.L)}
    for b in c.boundaries:
        out[f"band{b}"] = inside & (i0 // c.rows == b - 1) & (i1 // c.rows == b)
    return out


@pytest.mark.parametrize("load", pc.LOADS)
@pytest.mark.parametrize("cid", ALL)
def test_every_edge_class_is_present(cid, load):
    c = pc.CASES[cid]
    k = _classes(cid, load)
    counts = {name: int(m.sum()) for name, m in k.items()}
    print(cid, load, counts)
    # a reset folds every position into [0, L): nothing is dropped by x and none is L; an upload keeps both
    gone = ("inside", "slope") + (("drop_x", "x_is_L") if load == "reset" else ())
    want = SMALL.get(cid, [n for n in counts if n not in gone])
    if load == "reset":
        assert counts["drop_x"] == 0 and counts["x_is_L"] == 0
        assert not k["nonfinite"][np.isfinite(pc.state(cid)[1][0])].any()          # only a non-finite v is left
    for name in want:
        assert counts[name] > 0, (cid, name, counts)
    assert counts["inside"] > 0
    if cid in BIG:
        assert c.bands == 1 or len(c.boundaries) == min(c.bands - 1, 5)
        for e in range(c.E):
            if cid == "I" and e == 1:
                assert not _classes(cid, load, e)["inside"].any()          # every v above vmax
                continue
            ke = _classes(cid, load, e)
            assert 3 * ke["inside"].sum() >= c.N and 8 * ke["slope"].sum() >= c.N, (cid, e, ke["inside"].sum(), ke["slope"].sum())
    # a band straddler on the boundary itself gives both bands about half its weight (fx = 1/2 up to the rounding of x / dx)
    _, _, _, _, _, fx, _, _ = (a.numpy() for a in hp.locate(*(pc._t(a[0]) for a in pc.particles(cid, load)), c.grid()))
    for b in c.boundaries:
        assert (np.abs(fx[k[f"band{b}"]] - 0.5) < 1e-9).any(), (cid, b)
    # occupied bins meet feq = 0; empty bins exist where the grid is larger than the state
    f = pc.ref(cid, load)["f"]
    shared, per = pc.targets(cid)
    assert ((f[0] > 0) & (shared == 0)).any() and ((f > 0) & (per == 0)).any()
    if cid in ("D1", "D2", "E", "F", "G"):
        assert (f == 0).any(axis=(1, 2)).all()
    if cid == "I":
        X, V = pc.state(cid)
        assert np.array_equal(X[2], X[0], equal_nan=True) and np.array_equal(V[2], V[0], equal_nan=True)


@pytest.mark.parametrize("cid", ALL)
def test_state_is_deterministic_and_within_reach_of_reset(cid):
    c = pc.CASES[cid]
    X, V = pc.state(cid)
    X2, V2 = pc.state.__wrapped__(cid)                  # built again
    assert np.array_equal(X, X2, equal_nan=True) and np.array_equal(V, V2, equal_nan=True)
    assert X.shape == V.shape == (c.E, c.N)
    fin = np.isfinite(X)
    assert (X[fin] >= -c.L).all() and (X[fin] < 2 * c.L).all()      # no position beyond [-L, 2L) other than nan and inf
    Xr, Vr = pc.particles(cid, "reset")
    assert np.array_equal(Vr, V, equal_nan=True) and (Xr >= 0).all() and (Xr < c.L).all() and not np.signbit(Xr).any()
    inbox = fin & (X > 0) & (X < c.L)
    assert np.array_equal(Xr[inbox], X[inbox]) and not Xr[~fin].any() and not Xr[X == c.L].any()
    assert np.array_equal(pc.particles(cid, "set")[0], X, equal_nan=True)


@pytest.mark.parametrize("load", pc.LOADS)
@pytest.mark.parametrize("cid", ALL)
def test_reference_mass_is_exact(cid, load):
    c = pc.CASES[cid]
    G = c.grid()
    X, V = (pc._t(a) for a in pc.particles(cid, load))
    inside = hp.locate(X, V, G)[0]
    assert G.abits + G.bbits == 62 - max(1, c.N.bit_length())
    total = hp.counts(X, V, G).sum(dim=(1, 2))
    assert [int(t) for t in total] == [int(n) << (G.abits + G.bbits) for n in inside.sum(dim=1)]


def test_weight_bits_step_between_d1_and_d2():
    g1, g2 = pc.CASES["D1"].grid(), pc.CASES["D2"].grid()
    assert (g1.abits + g1.bbits, g2.abits + g2.bbits) == (54, 53)
    a = pc.CASES["A"].grid()
    assert a.abits + a.bbits == 61


@pytest.mark.parametrize("load", pc.LOADS)
@pytest.mark.parametrize("cid", ALL)
def test_reference_agrees_with_autograd_on_the_finite_substate(cid, load):
    """vjp_ld against hp_phase.autograd_vjp, and jvp_ld against torch forward mode through hp_phase.density_st, on the state with
    the non-finite particles replaced by dropped finite ones (autograd turns one NaN particle into NaN everywhere)."""
    import torch.autograd.forward_ad as fwAD
    c = pc.CASES[cid]
    G = c.grid()
    X, V = pc.finite_state(cid, load)
    bad = ~(np.isfinite(pc.particles(cid, load)[0]) & np.isfinite(pc.particles(cid, load)[1]))
    feq = pc.targets(cid)[1]
    d = np.asarray(c.d_kl)
    gx, gv = pc.vjp_ld(X, V, G, feq, d)
    ax, av = hp.autograd_vjp(pc._t(X), pc._t(V), pc._t(feq), pc._t(d), G)
    err = pc.grad_err(ax.numpy(), av.numpy(), (gx, gv))
    print(f"{cid} {load}: vjp_ld against autograd {err:.3e}")
    assert err <= 1e-12
    # replacing a non-finite particle by a dropped one changes nothing: the reference of the full state is the same numbers
    fx, fv = pc.ref(cid, load)["env"]["grad"]
    assert np.array_equal(fx, gx) and np.array_equal(fv, gv)
    assert not fx[bad].any() and not fv[bad].any()
    ux, uv = pc.vjp_ld(X, V, G, feq, np.ones(c.E))
    K = pc.ks(cid)[-1]
    tx, tv = pc.tangents(cid, K)
    want, S = pc.jvp_ld(ux, uv, tx, tv)
    for k in range(K):
        with fwAD.dual_level():
            xd, vd = fwAD.make_dual(pc._t(X), pc._t(tx[k])), fwAD.make_dual(pc._t(V), pc._t(tv[k]))
            t = fwAD.unpack_dual(hp.kl(hp.density_st(xd, vd, G), pc._t(feq), G)).tangent
            got = np.zeros(c.E) if t is None else t.numpy()
        ok = S[k] > 0
        assert (np.abs(got[ok] - want[k][ok]) <= 1e-12 * S[k][ok]).all(), (cid, k, got, want[k], S[k])
        assert not got[~ok].any()


@pytest.mark.parametrize("load", pc.LOADS)
@pytest.mark.parametrize("cid", ALL)
def test_floors_are_small(cid, load):
    fl = pc.floors(cid, load)
    print(f"{cid} {load}: floor kl {fl['kl']:.3e}  grad {fl['grad']:.3e}  bounds kl {pc.bound(cid, load, 'kl'):.3e}  "
          f"grad {pc.bound(cid, load, 'grad'):.3e}  jvp {pc.bound(cid, load, 'jvp'):.3e}")
    for v in fl.values():
        assert np.isfinite(v) and v < 1e-14
    for s in ("kl", "grad", "jvp"):
        assert 0 < pc.bound(cid, load, s) <= pc.CEILING
    r = pc.ref(cid, load)
    for name in ("shared", "env"):
        assert np.isfinite(r[name]["kl"].astype(np.float64)).all()
        assert all(np.isfinite(g.astype(np.float64)).all() for g in r[name]["grad"])


@pytest.mark.parametrize("load", pc.LOADS)
def test_exact_zeros_of_the_reference(load):
    """Where the device is held to exactly 0, the reference is exactly 0."""
    gx, gv = pc.ref("B", load)["env"]["grad"]
    assert not gx.any()                                # nx = 1: g_x exactly 0
    gx, gv = pc.ref("C", load)["env"]["grad"]
    assert not gv.any()                                # nv = 1: g_v exactly 0
    r = pc.ref("I", load)
    assert not r["f"][1].any() and r["env"]["kl"][1] == 0 and r["env"]["S_kl"][1] == 0
    for g in r["env"]["grad"]:
        assert not g[1].any() and not g[2].any()       # env 1 empty, env 2 with d_kl = 0
    assert r["unit"][0][2].any()


def test_rows_is_the_hosts_band_height():
    for c in pc.CASES.values():
        assert pc.rows(c.nx, c.nv) == min(c.nx, max(1, 65536 // (8 * c.nv)))
        assert c.rows * c.nv * 8 <= 65536
    f = pc.CASES["F"]
    assert (f.rows, f.bands, f.rows * f.nv * 8) == (8, 128, 65536)
    e, g = pc.CASES["E"], pc.CASES["G"]
    assert (e.rows, e.bands, e.nx - e.rows) == (8, 2, 1)           # the last band is one row
    assert (g.rows, g.bands) == (32, 8) and g.nx % g.rows != 0     # partial last band
    assert np.finfo(pc.LD).eps < 2e-19                             # the reference's precision: 80-bit or better
