"""The fluid moments and their derivatives on the device at the edge shapes, extreme velocity scales and special values of
tests/hp_moments_cases.py (pic_moments, pic_moments_vjp, pic_moments_jvp).

Parity is asserted per node against a bound derived from the header's integer units (hp_moments_cases.bound / jvp_bound): the
measured quantity is the ratio error / bound, which must not exceed 1; the max-normalised error of the older tests is recorded
beside it (moments_edges.*; profiles/moments_edges.md).  Everything else is bitwise: scale equivariance, the special values, the
independence of the batch, of blocks_per_env and of the number of directions in a call.  The premises (the references satisfy all
of it among themselves) are pinned by tests/test_moments_edges_cpu.py.  No handle is stepped.

Measured on an MI355X: error / bound 0.03 to 0.24 at cases B, C, E, F and under every profile, up to 0.55 at case A, 0.87 to
0.993 at case D (one particle per touched node: one term's rounding to the unit is the whole error, and the NumPy model of the
contract gives the same figures); pic_moments_jvp 0.13, 0.14, 0.28, 0.99, 0.07 at A to E; the gather 1.9e-16, 1.4e-16, 1.6e-15 at
A, B, C."""
import numpy as np
import pytest
import torch

import hp_moments as hm
import hp_moments_cases as mc
from conftest import record_measure

pytestmark = pytest.mark.gpu

LD = mc.LD
DUAL_BOUND = 7.8e-12          # tests/test_gpu_moments_jvp.py: DUAL_BOUND
BASE = [(cid, fmt, shape) for cid in mc.CASES for fmt in mc.FORMATS for shape in mc.SHAPES]
PROFILED = [(cid, fmt, p) for cid in mc.PROFILE_CASES for fmt in mc.FORMATS for p in mc.profiles(fmt)]
JVP_CASES = ("A", "B", "C", "D", "E")


def _ids(rows):
    return ["-".join(r) for r in rows]


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _make(cid, fmt="float64", shape="CIC", XV=None, bpe=0):
    """A handle of case cid holding the batch XV (default: every environment, base profile), with the case's L and n0; on a
    fixed32 handle the raw words of hp_moments_cases.RAW_WORDS are planted behind the reset."""
    from ocplasma_amd.env.batched import BatchedPIC
    c = mc.CASES[cid]
    X, V = mc.batch(cid, fmt) if XV is None else XV
    env = BatchedPIC(X.shape[0], c.N, c.mesh(fmt), n0=c.n0, L=c.L, dt=0.01, interpol=shape, blocks_per_env=bpe, **mc.FORMATS[fmt])
    assert env.n0 == c.n0 and env.L == c.L and env.N_mesh == c.mesh(fmt)
    _reset(env, cid, fmt, X, V)
    return env


def _reset(env, cid, fmt, X, V):
    env.reset(np.ascontiguousarray(X), np.ascontiguousarray(V))
    if fmt == "fixed32" and mc.CASES[cid].N >= 63:
        env.sync()
        xf = env.torch_views()["x_fixed"]
        for i, raw in mc.RAW_WORDS:
            xf[:, i] = raw - (1 << 32) if raw >= (1 << 31) else raw
        torch.cuda.synchronize()
        env.refresh()


def _held(env, fmt):
    """The particles as the device holds them: x (the particle dtype, wrapped as the reference project wraps; or the uint32 words
    of fixed positions) and v."""
    x, v = env.particles()
    if fmt == "fixed32":
        env.sync()
        x = env.torch_views()["x_fixed"].cpu().numpy().view(np.uint32)
        for i, raw in mc.RAW_WORDS if env.N >= 63 else ():
            assert np.all(x[:, i] == raw)
        return x, v
    return np.stack([mc.held(r, fmt, env.L) for r in x]), v


def _forward(env, cid, fmt, shape, profile, envs):
    """(worst error / bound, worst max-normalised error) of env.moments() over those of `envs` (the case's environment held at
    each place of the batch) that are reference environments; the special values of the profile are asserted on the way."""
    c = mc.CASES[cid]
    Ng, cell = c.mesh(fmt), mc.cell_dtype(fmt)
    x, v = _held(env, fmt)
    m = env.moments()
    assert m.shape == (len(envs), 3, Ng)
    worst = norm = 0.0
    for i, e in enumerate(envs):
        if e not in c.ref_envs:
            continue
        assert np.array_equal(v[i], mc.velocities(cid, e, fmt, profile))         # the handle holds what it was given
        ref = hm.moments_ld(x[i], v[i], Ng, c.L, c.n0, shape, cell)
        bnd = mc.bound(c, profile, ref, mc.node_terms(x[i], v[i], Ng, c.L, shape, cell), fmt, shape)
        rows = (0, 1, 2)
        if profile == "m2_at":
            assert np.all(_bits(m[i, 2]) == _bits(np.array(np.inf))), "m2 must be +inf on every node from max|v| = 2^511"
            rows = (0, 1)
        else:
            assert np.isfinite(m[i]).all()
        r, n = mc.check_rows(m[i], ref, bnd, rows)
        worst, norm = max(worst, r), max(norm, n)
    return worst, norm


def _record(name, ratio, norm):
    print(f"moments_edges.{name}: error / bound = {ratio:.3f}   max-normalised error = {norm:.3e}")
    record_measure(f"moments_edges.{name}.ratio", ratio)
    record_measure(f"moments_edges.{name}.norm", norm)


# ---- 1. forward parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,fmt,shape", BASE, ids=_ids(BASE))
def test_moments_lie_within_the_derived_bound_at_every_case(cid, fmt, shape):
    c = mc.CASES[cid]
    env = _make(cid, fmt, shape)
    ratio, norm = _forward(env, cid, fmt, shape, "base", range(c.E))
    env.close()
    _record(f"{cid}.{fmt}.{shape}.base", ratio, norm)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("cid,fmt,profile", PROFILED, ids=_ids(PROFILED))
def test_moments_lie_within_the_derived_bound_under_every_profile(cid, fmt, profile):
    c = mc.CASES[cid]
    worst = 0.0
    for shape in mc.SHAPES:
        env = _make(cid, fmt, shape, XV=mc.batch(cid, fmt, profile))
        ratio, norm = _forward(env, cid, fmt, shape, profile, range(c.E))
        env.close()
        _record(f"{cid}.{fmt}.{shape}.{profile}", ratio, norm)
        worst = max(worst, ratio)
    assert worst <= 1.0, worst


# ---- 2. m0 is the density, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES)
@pytest.mark.parametrize("cid", list(mc.CASES))
def test_m0_is_the_density_bit_for_bit_at_every_case(cid, shape):
    env = _make(cid, "float64", shape)
    assert _same(env.moments()[:, 0], env.fields()[0])
    env.close()


# ---- 3. scale equivariance, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(mc.FORMATS))
@pytest.mark.parametrize("cid", mc.PROFILE_CASES)
def test_scaling_the_velocities_by_a_power_of_two_scales_the_moments_bit_for_bit(cid, fmt):
    """The units follow the data's exponent and nothing else does: m1(ldexp(v, k)) = ldexp(m1(v), k), m2 with 2k, m0 unchanged, as
    int64 bit patterns (no result is subnormal at these scalings: tests/test_moments_edges_cpu.py)."""
    for shape in mc.SHAPES:
        X, V = mc.batch(cid, fmt)
        env = _make(cid, fmt, shape, XV=(X, V))
        base = env.moments()
        assert np.isfinite(base).all() and base[:, 1:].any()
        for k in mc.SCALINGS[fmt]:
            _reset(env, cid, fmt, X, mc.batch(cid, fmt, f"scaled:{k}")[1])
            m = env.moments()
            assert _same(m[:, 0], base[:, 0]), (shape, k)
            assert _same(m[:, 1], np.ldexp(base[:, 1], k)), (shape, k)
            assert _same(m[:, 2], np.ldexp(base[:, 2], 2 * k)), (shape, k)
        env.close()


# ---- 4. the edge of m2, an environment at rest and a NaN, side by side ----------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES)
@pytest.mark.parametrize("cid", mc.PROFILE_CASES)
def test_the_m2_edge_next_to_an_environment_at_rest_and_a_nan(cid, shape):
    c = mc.CASES[cid]
    x = mc.positions(cid, 0, "float64")
    v = mc.velocities(cid, 0, "float64")
    bad = v.copy()
    bad[c.N - 1] = np.nan
    profs = ("m2_below", None, None, "m2_at", "pow2_max", "pow2_below")
    V = np.stack([mc.velocities(cid, 0, "float64", "m2_below"), np.zeros_like(v), bad, mc.velocities(cid, 0, "float64", "m2_at"),
                  mc.velocities(cid, 0, "float64", "pow2_max"), mc.velocities(cid, 0, "float64", "pow2_below")])
    env = _make(cid, "float64", shape, XV=(np.stack([x] * len(V)), V))
    m = env.moments()
    xh, vh = _held(env, "float64")
    for i, p in enumerate(profs):
        if p is None:
            continue
        ref = hm.moments_ld(xh[i], vh[i], c.Ng, c.L, c.n0, shape, np.float64)
        bnd = mc.bound(c, p, ref, mc.node_terms(xh[i], vh[i], c.Ng, c.L, shape, np.float64), "float64", shape)
        if p == "m2_at":
            assert np.all(_bits(m[i, 2]) == _bits(np.array(np.inf)))          # +inf on every node, the empty ones included
            ratio, norm = mc.check_rows(m[i], ref, bnd, (0, 1))
        else:
            assert np.isfinite(m[i]).all()                                    # nextafter(2^511, 0): m2 is finite
            ratio, norm = mc.check_rows(m[i], ref, bnd)
        _record(f"{cid}.float64.{shape}.batch_{p}", ratio, norm)
        assert ratio <= 1.0, (p, ratio)
    assert not _bits(m[1, 1:]).any()                                          # at rest: +0
    assert np.isnan(m[2, 1:]).all()                                           # the NaN stays in m1, m2 of its environment
    for i in range(1, len(V)):
        assert _same(m[i, 0], m[0, 0]), i                                     # m0 sees no velocity
    env.close()


# ---- 5. independence of the batch, of the call and of the grid --------------------------------------------------------------------
@pytest.mark.parametrize("fmt,shape", [("float64", "CIC"), ("float64", "TSC"), ("float32", "CIC"), ("fixed32", "TSC")])
def test_environments_at_very_different_scales_do_not_see_each_other(fmt, shape):
    cid, c = "C", mc.CASES["C"]
    x = mc.positions(cid, 0, fmt)
    v = mc.velocities(cid, 0, fmt)
    lo, hi = (-400, 480) if fmt == "float64" else (-100, 100)
    bad = v.copy()
    bad[5] = -np.inf
    V = np.stack([mc.velocities(cid, 0, fmt, f"scaled:{lo}"), v, mc.velocities(cid, 0, fmt, f"scaled:{hi}"), np.zeros_like(v), bad])
    X = np.stack([x] * len(V))
    env = _make(cid, fmt, shape, XV=(X, V))
    m = env.moments()
    assert _same(env.moments(), m)              # the max words and accumulators were cleared behind the read
    assert _same(env.moments_torch(), m)
    env.close()
    assert np.isfinite(m[:3]).all() and not _bits(m[3, 1:]).any() and np.isnan(m[4, 1:]).all() and np.isfinite(m[4, 0]).all()
    assert _same(m[0, 1], np.ldexp(m[1, 1], lo)) and _same(m[2, 2], np.ldexp(m[1, 2], 2 * hi))
    for i in range(len(V)):
        alone = _make(cid, fmt, shape, XV=(X[i:i + 1], V[i:i + 1]))
        assert _same(alone.moments()[0], m[i]), i
        alone.close()


def test_case_E_gives_the_same_bits_whatever_blocks_per_env():
    got = []
    for bpe in (0, 3, 7):
        env = _make("E", "float64", "CIC", bpe=bpe)
        got.append(env.moments())
        env.close()
    assert _same(got[1], got[0]) and _same(got[2], got[0])


def test_case_F_first_and_last_environment_hold_the_same_particles_and_give_the_same_bits():
    c = mc.CASES["F"]
    for fmt in ("float64", "fixed32"):
        env = _make("F", fmt, "CIC")
        m = env.moments()
        env.close()
        assert _same(m[c.E - 1], m[0]) and not _same(m[c.E - 2], m[0])
        alone = _make("F", fmt, "CIC", XV=mc.batch("F", fmt, envs=[c.E - 1]))
        assert _same(alone.moments()[0], m[c.E - 1])
        alone.close()


# ---- 6. the forward mode (float64, CIC) ---------------------------------------------------------------------------------------------
def _dyadic_tangent(c, e):
    """d_x [N] with d_x / dx = q 2^-10 exactly in float64, q integers in [-1023, 1023] (0 where no neighbouring double divides
    exactly), and q: every dm0 term is then q 2^-10 cells exactly and dm0 can be checked as integers."""
    rng = np.random.default_rng([c.N, c.Ng, c.salt, e, 7])
    q = rng.integers(-1023, 1024, c.N)
    q[0] = 1023
    dx = c.L / c.Ng
    t = q * 2.0 ** -10
    d = t * dx
    for cand in (np.nextafter(d, np.inf), np.nextafter(d, -np.inf)):
        fix = (d / dx != t) & (cand / dx == t)
        d[fix] = cand[fix]
    miss = d / dx != t
    d[miss], q[miss] = 0.0, 0
    return d, q


@pytest.mark.parametrize("cid", JVP_CASES)
def test_jvp_lies_within_its_derived_bound_and_dm0_sums_to_zero(cid):
    c = mc.CASES[cid]
    env = _make(cid)
    xh, v = _held(env, "float64")
    T = [mc.tangents(cid, e) for e in range(c.E)]
    d_x, d_v = np.stack([t[0] for t in T]), np.stack([t[1] for t in T])
    got = env.moments_jvp(d_x, d_v)
    only_x, only_v = env.moments_jvp(d_x=d_x), env.moments_jvp(d_v=d_v)
    worst = norm = 0.0
    for e in range(c.E):
        for g, tx, tv in ((got, d_x[e], d_v[e]), (only_x, d_x[e], None), (only_v, None, d_v[e])):
            ref = mc.jvp_ld(xh[e], v[e], tx, tv, c.Ng, c.L, c.n0)
            r, n = mc.check_rows(g[e], ref, mc.jvp_bound(c, ref, xh[e], v[e], tx, tv))
            worst, norm = max(worst, r), max(norm, n)
        # sum_j dm0_j = 0: exact in the integers; every double carries the conversion's and the scale's rounding
        s0 = got[e, 0].astype(LD)
        assert abs(float(s0.sum())) <= 2 * mc.U64 * float(np.abs(s0).sum())
    assert not _bits(only_v[:, 0]).any()
    # ... and as integers: with iota = q 2^-10 exactly, dm0_j / s 2^10 is the integer sum_right q - sum_left q of node j
    D = [_dyadic_tangent(c, e) for e in range(c.E)]
    dm0 = env.moments_jvp(d_x=np.stack([d for d, _ in D]))[:, 0]
    s = c.n0 * c.L / c.N / (c.L / c.Ng)
    for e in range(c.E):
        q = D[e][1]
        k = dm0[e].astype(LD) / LD(s) * 1024
        assert float(np.max(np.abs(k - np.rint(k)))) < 1e-3
        jf = np.floor(xh[e] / (c.L / c.Ng)).astype(np.int64)
        want = np.bincount(np.mod(jf + 1, c.Ng), q, c.Ng) - np.bincount(np.mod(jf, c.Ng), q, c.Ng)
        assert np.array_equal(np.rint(k).astype(np.int64), want.astype(np.int64)) and int(np.rint(k).sum()) == 0
    env.close()
    _record(f"jvp.{cid}", worst, norm)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("cid", ["B", "C"])
def test_eight_directions_in_one_call_keep_to_themselves(cid):
    """Scales 2^-300, 1, 2^300 of one tangent, all-zero, d_x only, d_v only, one with a NaN, and an ordinary one: every direction's
    rows are those of a call of its own, the scaled ones ldexp of the unscaled, and the NaN stays where it is."""
    c = mc.CASES[cid]
    env = _make(cid)
    T = [mc.tangents(cid, e) for e in range(c.E)]
    tx, tv = np.stack([t[0] for t in T]), np.stack([t[1] for t in T])
    z = np.zeros_like(tx)
    other = np.random.default_rng([c.N, c.Ng, 99]).standard_normal((2,) + tx.shape)
    nanv = tv.copy()
    nanv[1, 7 % c.N] = np.nan
    d_x = np.stack([np.ldexp(tx, -300), tx, np.ldexp(tx, 300), z, tx, z, tx, other[0]])
    d_v = np.stack([np.ldexp(tv, -300), tv, np.ldexp(tv, 300), z, z, tv, nanv, other[1]])
    got = env.moments_jvp(d_x, d_v)
    assert got.shape == (8, c.E, 3, c.Ng)
    for k in range(8):
        assert _same(env.moments_jvp(d_x[k], d_v[k]), got[k]), k
    assert np.isfinite(got[:6]).all() and got[1].any()
    assert _same(got[0], np.ldexp(got[1], -300)) and _same(got[2], np.ldexp(got[1], 300))
    assert not _bits(got[3]).any()
    assert not _bits(got[5][:, 0]).any() and _same(got[4][:, 0], got[1][:, 0])
    assert _same(got[4], env.moments_jvp(d_x=tx)) and _same(got[5], env.moments_jvp(d_v=tv))
    assert np.isnan(got[6, 1, 1:]).all() and _same(got[6, 1, 0], got[1, 1, 0])       # dm0 does not see d_v
    keep = [e for e in range(c.E) if e != 1]
    assert _same(got[6][keep], got[1][keep])
    assert _same(env.moments_jvp(d_x, d_v), got)                                      # cleared behind the NaN
    env.close()


@pytest.mark.parametrize("cid", ["B", "C"])
def test_scaling_v_and_d_v_alike_scales_the_tangents_bit_for_bit(cid):
    c = mc.CASES[cid]
    X, V = mc.batch(cid, "float64")
    T = [mc.tangents(cid, e) for e in range(c.E)]
    tx, tv = np.stack([t[0] for t in T]), np.stack([t[1] for t in T])
    env = _make(cid, XV=(X, V))
    base = env.moments_jvp(tx, tv)
    assert np.isfinite(base).all()
    for k in (-400, 400):
        _reset(env, cid, "float64", X, np.ldexp(V, k))
        got = env.moments_jvp(tx, np.ldexp(tv, k))
        assert _same(got[:, 0], base[:, 0]), k
        assert _same(got[:, 1], np.ldexp(base[:, 1], k)) and _same(got[:, 2], np.ldexp(base[:, 2], 2 * k)), k
    env.close()


# ---- 7. the gather, called directly -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mc.VJP_CASES)
def test_vjp_matches_the_longdouble_gather_at_the_planted_positions(cid):
    c = mc.CASES[cid]
    env = _make(cid)
    xh, v = _held(env, "float64")
    g = np.stack([mc.tangents(cid, e)[2] for e in range(c.E)])
    gx, gv = env.moments_vjp(g)
    bound = mc.vjp_bound(cid)
    worst = 0.0
    for e in range(c.E):
        for got, want in zip((gx[e], gv[e]), mc.vjp_ld(xh[e], v[e], g[e], c.Ng, c.L, c.n0)):
            den = float(np.linalg.norm(want.astype(np.float64)))
            worst = max(worst, float(np.linalg.norm((got.astype(LD) - want).astype(np.float64))) / max(den, 1e-300))
    print(f"moments_edges.vjp.{cid}: device {worst:.3e}  floor {mc.vjp_floor(cid):.3e}  bound {bound:.3e}")
    record_measure(f"moments_edges.vjp.{cid}", worst)
    assert worst <= bound, worst
    if cid == "C":                              # duality with the device's forward mode, the gather from the reference
        T = [mc.tangents(cid, e) for e in range(c.E)]
        jm = env.moments_jvp(np.stack([t[0] for t in T]), np.stack([t[1] for t in T]))
        dual = 0.0
        for e in range(c.E):
            rx, rv = mc.vjp_ld(xh[e], v[e], g[e], c.Ng, c.L, c.n0)
            lhs = float((g[e].astype(LD) * jm[e].astype(LD)).sum())
            rhs = float((rx * T[e][0]).sum() + (rv * T[e][1]).sum())
            dual = max(dual, abs(lhs - rhs) / abs(rhs))
        record_measure("moments_edges.duality.C", dual)
        assert dual < DUAL_BOUND, dual
    env.close()
