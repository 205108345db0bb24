"""The premises of tests/test_gpu_moments_edges.py, on the references alone (no device): everything the GPU tests assert of the
device must already hold between the longdouble references (hp_moments.moments_ld, hp_moments_jvp.jvp_ld), the NumPy restatement
of the header's integer contract (hp_moments_cases.quantised_moments / quantised_jvp) and the derived bounds."""
import numpy as np
import pytest

import hp_moments as hm
import hp_moments_cases as mc
import hp_reference as hr
from conftest import record_measure

LD = mc.LD
ALL = [(cid, fmt, shape) for cid in mc.CASES for fmt in mc.FORMATS for shape in mc.SHAPES]
PROFILED = [(cid, fmt, p) for cid in mc.PROFILE_CASES for fmt in mc.FORMATS for p in mc.profiles(fmt)]
DIR_SCALES = (-300, 0, 300)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _held(cid, e, fmt):
    c = mc.CASES[cid]
    return mc.words_of(cid, e) if fmt == "fixed32" else mc.held(mc.positions(cid, e, fmt), fmt, c.L)


def _model_ratio(cid, fmt, shape, profile):
    """Worst |quantised - longdouble| / bound over the reference environments; the special values are asserted on the way."""
    c = mc.CASES[cid]
    Ng, cell = c.mesh(fmt), mc.cell_dtype(fmt)
    worst = 0.0
    for e in c.ref_envs:
        xh, v = _held(cid, e, fmt), mc.velocities(cid, e, fmt, profile)
        ref = hm.moments_ld(xh, v, Ng, c.L, c.n0, shape, cell)
        q = mc.quantised_moments(xh, v, Ng, c.L, c.n0, shape, cell)
        bnd = mc.bound(c, profile, ref, mc.node_terms(xh, v, Ng, c.L, shape, cell), fmt, shape)
        rows = (0, 1) if profile == "m2_at" else (0, 1, 2)
        if profile == "m2_at":
            assert np.all(q[2] == np.inf)
        else:
            assert np.isfinite(q).all()
        worst = max(worst, mc.check_rows(q, ref, bnd, rows)[0])
    return worst


@pytest.mark.parametrize("cid,fmt,shape", ALL, ids=["-".join(a) for a in ALL])
def test_the_quantised_model_lies_within_the_bound_at_every_case(cid, fmt, shape):
    r = _model_ratio(cid, fmt, shape, "base")
    print(f"moments_edges.model.{cid}.{fmt}.{shape}.base = {r:.3f}")
    record_measure(f"moments_edges.model.{cid}.{fmt}.{shape}.base", r)
    assert r <= 1.0, r


@pytest.mark.parametrize("cid,fmt,profile", PROFILED, ids=["-".join(a) for a in PROFILED])
def test_the_quantised_model_lies_within_the_bound_under_every_profile(cid, fmt, profile):
    worst = max(_model_ratio(cid, fmt, shape, profile) for shape in mc.SHAPES)
    print(f"moments_edges.model.{cid}.{fmt}.{profile} = {worst:.3f}")
    record_measure(f"moments_edges.model.{cid}.{fmt}.{profile}", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("fmt", list(mc.FORMATS))
@pytest.mark.parametrize("cid", mc.PROFILE_CASES)
def test_scaling_the_velocities_scales_the_references_exactly(cid, fmt):
    """scaled:k is exact in the particle dtype; moments_ld(x, ldexp(v, k)) is ldexp of the unscaled rows by k and 2k, bit for bit in
    longdouble; the quantised model is bit-equivariant in float64 (the units move with the data, nothing else does)."""
    c = mc.CASES[cid]
    Ng, cell = c.mesh(fmt), mc.cell_dtype(fmt)
    for e in c.ref_envs:
        xh, v = _held(cid, e, fmt), mc.velocities(cid, e, fmt)
        ref = hm.moments_ld(xh, v, Ng, c.L, c.n0, "CIC", cell)
        q = mc.quantised_moments(xh, v, Ng, c.L, c.n0, "CIC", cell)
        for k in mc.SCALINGS[fmt]:
            vk = mc.velocities(cid, e, fmt, f"scaled:{k}")
            assert vk.dtype == v.dtype and np.array_equal(hr.as_ld(vk), np.ldexp(hr.as_ld(v), k))
            assert np.all(np.abs(vk[v != 0]) >= np.finfo(v.dtype).tiny)       # no subnormal input
            rk = hm.moments_ld(xh, vk, Ng, c.L, c.n0, "CIC", cell)
            assert np.array_equal(rk[0], ref[0])
            assert np.array_equal(rk[1], np.ldexp(ref[1], k)) and np.array_equal(rk[2], np.ldexp(ref[2], 2 * k))
            qk = mc.quantised_moments(xh, vk, Ng, c.L, c.n0, "CIC", cell)
            assert np.array_equal(_bits(qk[0]), _bits(q[0]))
            assert np.array_equal(_bits(qk[1]), _bits(np.ldexp(q[1], k)))
            assert np.array_equal(_bits(qk[2]), _bits(np.ldexp(q[2], 2 * k)))
            # every scaled result is a normal float64: the equivariance asserted on the device cannot meet a subnormal
            nz = qk[1:][qk[1:] != 0]
            assert np.isfinite(nz).all() and np.all(np.abs(nz) >= np.finfo(np.float64).tiny)
            # 2e + b - 61 stays inside the exponent range (the issue's condition on the scalings)
            ex = mc.exponent_above(float(np.max(np.abs(vk.astype(np.float64)))))
            assert ex <= 511 and 2 * ex + mc.bits_of(c.N) - 61 > -1022


@pytest.mark.parametrize("cid", mc.PROFILE_CASES)
def test_the_profiles_have_the_properties_their_names_claim(cid):
    c = mc.CASES[cid]
    for e in c.ref_envs:
        for fmt in mc.FORMATS:
            v = mc.velocities(cid, e, fmt).astype(np.float64)
            top = lambda p: float(np.max(np.abs(mc.velocities(cid, e, fmt, p).astype(np.float64))))  # noqa: E731
            assert np.max(np.abs(v)) < 16 and np.count_nonzero(v) == c.N
            out = mc.velocities(cid, e, fmt, "outlier").astype(np.float64)
            assert top("outlier") == 2.0 ** 40 and mc.exponent_above(top("outlier")) == 41
            assert np.count_nonzero(out != v) == 1                       # the rest unscaled
            assert np.all(mc.velocities(cid, e, fmt, "negative") < 0)
            assert top("pow2_max") == 4.0 and mc.exponent_above(top("pow2_max")) == 3
            assert top("pow2_below") < 4.0 and mc.exponent_above(top("pow2_below")) == 2
            assert top("pow2_below") == float(np.nextafter(np.dtype(mc.FORMATS[fmt]["dtype"]).type(4), 0))
            for p in ("pow2_max", "pow2_below"):
                assert np.count_nonzero(np.abs(mc.velocities(cid, e, fmt, p).astype(np.float64)) == top(p)) == 1
        xh = _held(cid, e, "float64")
        for p, state in (("m2_below", "ok"), ("m2_at", "inf2")):
            v = mc.velocities(cid, e, "float64", p)
            assert mc.unit_state(float(np.max(np.abs(v)))) == state
            assert mc.exponent_above(float(np.max(np.abs(v)))) == (511 if state == "ok" else 512)
            assert np.count_nonzero(np.abs(v) >= 16) == 1                # the rest O(1)
            q = mc.quantised_moments(xh, v, c.Ng, c.L, c.n0)
            assert np.isfinite(q[:2]).all() and (np.isfinite(q[2]).all() if state == "ok" else np.all(q[2] == np.inf))
            # (the finite m2 needs s < 1: v^2 itself is just below the largest double)
            assert c.n0 * c.Ng / c.N < 1
        # at rest and non-finite: +0 and NaN in m1, m2; m0 untouched
        v = mc.velocities(cid, e, "float64")
        q = mc.quantised_moments(xh, v, c.Ng, c.L, c.n0)
        rest = mc.quantised_moments(xh, np.zeros_like(v), c.Ng, c.L, c.n0)
        bad = v.copy()
        bad[3] = np.nan
        nanq = mc.quantised_moments(xh, bad, c.Ng, c.L, c.n0)
        assert not _bits(rest[1:]).any() and np.isnan(nanq[1:]).all()
        assert np.array_equal(_bits(rest[0]), _bits(q[0])) and np.array_equal(_bits(nanq[0]), _bits(q[0]))


def test_the_outlier_coarsens_its_environment_and_the_bound_says_so():
    """One particle at 2^40 among velocities of order 1: the units of m1 / m2 are 2^40 / 2^80 times coarser, and the bound at a node
    the fast particle does not touch grows accordingly (the header's 'N 2^-61 of N max|v|', not a flat fraction of the largest
    node)."""
    cid, c = "C", mc.CASES["C"]
    xh = _held(cid, 0, "float64")
    out = []
    for p in ("base", "outlier"):
        v = mc.velocities(cid, 0, "float64", p)
        ref = hm.moments_ld(xh, v, c.Ng, c.L, c.n0)
        out.append(mc.bound(c, p, ref, mc.node_terms(xh, v, c.Ng, c.L)))
    base, outl = out
    e0 = mc.exponent_above(float(np.max(np.abs(mc.velocities(cid, 0, "float64")))))
    far = int(np.argmin(outl[2]))                # a node without the fast particle
    # (the base bound is led by the weights' own error, (2 Ng + 4) u64 per term, about 2^6 half units of m1: hence the margins)
    assert float(outl[1][far] / base[1][far]) > 2.0 ** (41 - e0 - 8)
    assert float(outl[2][far] / base[2][far]) > 2.0 ** (2 * (41 - e0) - 16)


def test_the_draws_of_case_F_do_not_collide():
    c = mc.CASES["F"]
    assert c.ref_envs[0] == 0 and c.ref_envs[-1] == c.E - 1 and len(set(c.ref_envs)) == 5
    seen = {}
    for e in range(c.E - 1):
        key = (mc.positions("F", e, "float64")[100:].tobytes(), mc.velocities("F", e, "float64").tobytes())
        assert key not in seen, (e, seen[key])
        seen[key] = e
    for fmt in mc.FORMATS:                       # the last environment repeats the first
        assert np.array_equal(mc.positions("F", c.E - 1, fmt), mc.positions("F", 0, fmt))
        assert np.array_equal(mc.velocities("F", c.E - 1, fmt), mc.velocities("F", 0, fmt))


def test_planted_positions_are_where_they_should_be():
    for cid, c in mc.CASES.items():
        for fmt in mc.FORMATS:
            x = mc.positions(cid, 0, fmt)
            assert x.dtype == np.dtype(mc.FORMATS[fmt]["dtype"])
            if c.N < 63:
                continue
            assert x[0] == 0 and not np.signbit(x[0]) and x[1] == 0 and np.signbit(x[1])
            assert x[2] == np.nextafter(x.dtype.type(c.L), x.dtype.type(0)) and np.all(x[3:6] < 0)
            xh = mc.held(x, fmt if fmt != "fixed32" else "float32", c.L)
            assert np.all((xh >= 0) & (xh < c.L)) and np.all(xh[3:5] == 0)      # (the wrap rounds the tiniest negatives onto 0)
            dxw = x.dtype.type(c.L / c.mesh(fmt))
            on = x[6:30] / dxw
            assert np.allclose(on, np.round(on), atol=1e-3)              # k dx; the next 48 are its two neighbours
        w = mc.words_of(cid, 0)
        if c.N >= 63:
            assert w.dtype == np.uint32 and w[0] == 0 and w[1] == 0xFFFFFFFF


@pytest.mark.parametrize("cid", ["A", "B", "C", "D", "E"])
def test_the_jvp_model_lies_within_its_bound_and_scales_exactly(cid):
    c = mc.CASES[cid]
    worst = 0.0
    for e in c.ref_envs:
        xh, v = _held(cid, e, "float64"), mc.velocities(cid, e, "float64")
        d_x, d_v, _ = mc.tangents(cid, e)
        base = None
        for k in DIR_SCALES:
            tx, tv = np.ldexp(d_x, k), np.ldexp(d_v, k)
            ref = mc.jvp_ld(xh, v, tx, tv, c.Ng, c.L, c.n0)
            q = mc.quantised_jvp(xh, v, tx, tv, c.Ng, c.L, c.n0)
            bnd = mc.jvp_bound(c, ref, xh, v, tx, tv)
            worst = max(worst, mc.check_rows(q, ref, bnd)[0])
            s0 = q[0].astype(LD)                 # exact in the integers; the doubles carry the conversion and the scale
            assert abs(float(s0.sum())) <= 2 * mc.U64 * float(np.abs(s0).sum())
            if k == 0:
                base, base_ref = q, ref
        for k in DIR_SCALES:                     # the directions' scales move the units, nothing else
            q = mc.quantised_jvp(xh, v, np.ldexp(d_x, k), np.ldexp(d_v, k), c.Ng, c.L, c.n0)
            assert np.array_equal(_bits(q), _bits(np.ldexp(base, k)))
            assert np.array_equal(mc.jvp_ld(xh, v, np.ldexp(d_x, k), np.ldexp(d_v, k), c.Ng, c.L, c.n0), np.ldexp(base_ref, k))
        # d_x alone, d_v alone, all zero
        only_v = mc.quantised_jvp(xh, v, None, d_v, c.Ng, c.L, c.n0)
        assert not _bits(only_v[0]).any()
        assert not _bits(mc.quantised_jvp(xh, v, np.zeros_like(d_x), None, c.Ng, c.L, c.n0)).any()
        for tx, tv in ((d_x, None), (None, d_v)):
            ref = mc.jvp_ld(xh, v, tx, tv, c.Ng, c.L, c.n0)
            q = mc.quantised_jvp(xh, v, tx, tv, c.Ng, c.L, c.n0)
            worst = max(worst, mc.check_rows(q, ref, mc.jvp_bound(c, ref, xh, v, tx, tv))[0])
        # velocities and d_v scaled alike: dm0 unchanged, dm1 2^k, dm2 2^(2k)
        for k in (-400, 400):
            q = mc.quantised_jvp(xh, np.ldexp(v, k), d_x, np.ldexp(d_v, k), c.Ng, c.L, c.n0)
            assert np.array_equal(_bits(q[0]), _bits(base[0])) and np.array_equal(_bits(q[1]), _bits(np.ldexp(base[1], k)))
            assert np.array_equal(_bits(q[2]), _bits(np.ldexp(base[2], 2 * k)))
        bad = d_v.copy()
        bad[0] = np.nan
        q = mc.quantised_jvp(xh, v, d_x, bad, c.Ng, c.L, c.n0)
        assert np.isnan(q[1:]).all() and np.array_equal(_bits(q[0]), _bits(base[0]))
    print(f"moments_edges.model.jvp.{cid} = {worst:.3f}")
    record_measure(f"moments_edges.model.jvp.{cid}", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("cid", mc.VJP_CASES)
def test_the_vjp_references_agree_and_the_bound_stays_under_the_ceiling(cid):
    import hp_adjoint as ha
    c = mc.CASES[cid]
    fl = mc.vjp_floor(cid)
    b = mc.vjp_bound(cid)
    record_measure(f"moments_edges.vjp_floor.{cid}", fl)
    assert fl < 1e-13 and b <= mc.VJP_CEILING
    S = ha.Setup(c.N, c.Ng, c.L, c.n0, 0.1)
    for e in c.ref_envs:                         # the longdouble gather is the float64 hand equations, more precisely
        x, v = mc.positions(cid, e, "float64"), mc.velocities(cid, e, "float64")
        g = mc.tangents(cid, e)[2]
        want = mc.vjp_ld(mc.held(x, "float64", c.L), v, g, c.Ng, c.L, c.n0)
        for a, w in zip(hm.hand_vjp(x, v, g, S), want):
            assert np.linalg.norm((a - w).astype(np.float64)) <= b * np.linalg.norm(w.astype(np.float64))
        # duality of the two longdouble references at this state
        d_x, d_v, _ = mc.tangents(cid, e)
        jm = mc.jvp_ld(mc.held(x, "float64", c.L), v, d_x, d_v, c.Ng, c.L, c.n0)
        lhs, rhs = (hr.as_ld(g) * jm).sum(), (want[0] * d_x).sum() + (want[1] * d_v).sum()
        assert abs(float(lhs - rhs)) <= 1e-15 * float(np.abs(hr.as_ld(g) * jm).sum())
