"""The device sampler (pic_reset_sampled) against its bit-level restatement, tests/hp_sampler.py.

x is IEEE arithmetic under -ffp-contract=off and must match bit for bit.  v goes through log, sqrt, sincospi and sin, which are
not correctly rounded on the device: it is compared with the longdouble twin within hp_sampler.velocity_bound.  The one allowed
difference is an accept / reject decision taken on a proposal within its own bound of +-10; those particles are counted
(record_measure) and left out of the value comparison."""

import numpy as np
import pytest

import hp_sampler as hs
from conftest import record_measure

pytestmark = pytest.mark.gpu

KINDS = {"two-stream": 0, "bump-on-tail": 1}
_NEAR = {"count": 0}


def _device_state(env, fmt):
    views = env.torch_views()
    env.sync()
    if fmt == "fixed32":
        x = views["x_fixed"].cpu().numpy().view(np.uint32).copy()
    else:
        x = views["x"].cpu().numpy().copy()
    return x, views["v"].cpu().numpy().copy()


def _check_env(x_dev, v_dev, twin, A, fmt, tag):
    want_x = twin["x"]
    assert np.array_equal(x_dev.view(np.uint8), np.asarray(want_x).astype(x_dev.dtype).view(np.uint8)), (tag, "x")
    near = hs.decisions_near_edge(twin)
    tail = twin["attempt"] > hs.ATTEMPTS
    ok = ~near & ~tail
    b = hs.velocity_bound(twin, A, fmt)
    err = np.abs(v_dev.astype(np.float64) - twin["v"].astype(np.float64))
    if not np.all(err[ok] <= b[ok]):
        k = np.flatnonzero(ok)[np.argmax(err[ok] / b[ok])]
        raise AssertionError((tag, "v", float(err[k] / b[k]), "worst particle", int(k), "mu", float(twin["mu"][k]),
                              "v_raw", float(twin["v_raw"][k]), "r", float(twin["r"][k]), "err", float(err[k]), "bound", float(b[k])))
    r = float(np.max(err[ok] / b[ok])) if ok.any() else 0.0
    _NEAR["count"] += int(near.sum())
    record_measure("sampler_v_over_bound", max(r, _WORST.get("v", 0.0)))
    _WORST["v"] = max(r, _WORST.get("v", 0.0))
    record_measure("sampler_decisions_near_edge", _NEAR["count"])
    return near, tail


_WORST = {}


CASES = [
    # (fmt, kind, N, envs, env_base, seed, a, v0, sigma, A, L)
    ("float64", "two-stream", 1, 2, 0, 7, 0.0, 3.0, 1.0, 0.1, 50.0),
    ("float64", "bump-on-tail", 100003, 3, 5, 7, 0.2, 4.0, 0.5, 0.1, 50.0),
    ("float32", "two-stream", 4097, 2, 0, 7 + (1 << 32), 0.0, 4.0, 0.5, 0.0, 77.7),
    ("float32", "bump-on-tail", 65537, 2, 1000, 123456789, 0.3, 5.0, 1.0, 0.2, 10.0),
    ("fixed32", "two-stream", 999, 2, 3, 2 ** 63 + 11, 0.0, 2.0, 0.7, 0.05, 1.0),
    ("fixed32", "bump-on-tail", 200001, 2, 0, 99, 0.2, 3.0, 1.0, 0.1, 50.0),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-N{c[2]}" for c in CASES])
def test_sampler_matches_restatement(case):
    import ocplasma_amd as oc
    fmt, kind, N, envs, base, seed, a, v0, sigma, A, L = case
    dtype = "float64" if fmt == "float64" else "float32"
    env = oc.BatchedPIC(envs, N, 64, L=L, dt=0.05, dtype=dtype, position_dtype="fixed32" if fmt == "fixed32" else None,
                        env_index_base=base)
    try:
        env.reset_sampled(kind, a=a, v0=v0, sigma=sigma, A=A, n_mode=3, seed=seed)
        x, v = _device_state(env, fmt)
        assert env.bad_count() == 0
    finally:
        env.close()
    for e in range(envs):
        twin = hs.sample(N, L, KINDS[kind], a, v0, sigma, A, 3, seed, base + e, fmt, ld=True)
        _check_env(x[e], v[e], twin, A, fmt, (case, e))
    # environments differ from each other
    if envs > 1 and N > 1:
        assert not np.array_equal(x[0], x[1])


def test_seeds_differing_only_in_the_high_word():
    import ocplasma_amd as oc
    N, L = 5000, 50.0
    out = []
    for seed in (42, 42 + (1 << 32)):
        env = oc.BatchedPIC(1, N, 64, L=L, dt=0.05)
        try:
            env.reset_sampled("bump-on-tail", seed=seed)
            x, v = _device_state(env, "float64")
        finally:
            env.close()
        twin = hs.sample(N, L, 1, 0.2, 3.0, 1.0, 0.1, 2, seed, 0, "float64", ld=True)
        _check_env(x[0], v[0], twin, 0.1, "float64", seed)
        out.append(x[0])
    assert not np.array_equal(out[0], out[1])


@pytest.mark.parametrize("fmt", ["float64", "float32", "fixed32"])
def test_exhausted_draws_stay_in_the_support(fmt):
    """Bump-on-tail with v0 = 12, sigma = 1: only Phi(-2) = 2.3 % of the beam lies in [-10, 10], so about 23 % of the beam
    particles reject all 63 Box-Muller proposals.  They must still lie in [-10, 10], drawn from the truncated normal: their
    values against scipy's truncnorm.ppf of the same uniform, and the whole beam KS-tested against truncnorm.  Every particle
    that accepts within 63 attempts stays what the restatement says, bit for bit in x and within the bound in v."""
    from scipy import stats
    import ocplasma_amd as oc
    N, L, a, v0, sigma = 200000, 50.0, 0.2, 12.0, 1.0
    dtype = "float64" if fmt == "float64" else "float32"
    env = oc.BatchedPIC(1, N, 64, L=L, dt=0.05, dtype=dtype, position_dtype="fixed32" if fmt == "fixed32" else None)
    try:
        env.reset_sampled("bump-on-tail", a=a, v0=v0, sigma=sigma, A=0.0, seed=31)
        x, v = _device_state(env, fmt)
    finally:
        env.close()
    v = v[0].astype(np.float64)
    assert np.all(np.abs(v) <= hs.VMAX), ("velocities outside [-10, 10]", int(np.sum(np.abs(v) > hs.VMAX)))
    twin = hs.sample(N, L, 1, a, v0, sigma, 0.0, 2, 31, 0, fmt, ld=True)
    near, tail = _check_env(x[0], v, twin, 0.0, fmt, fmt)
    nf = hs.n_first(1, N, a)
    record_measure(f"sampler_exhausted_{fmt}", int(tail.sum()))
    assert 0.2 * (N - nf) < tail.sum() < 0.26 * (N - nf)
    lo, hi = (-hs.VMAX - v0) / sigma, (hs.VMAX - v0) / sigma
    t = tail & ~near
    want = stats.truncnorm.ppf(twin["u_tail"][t], lo, hi, loc=v0, scale=sigma)
    u = hs.U64 if fmt == "float64" else hs.U32
    err = np.abs(v[t] - want)
    # normcdf / normcdfinv a few ulp each: at v = v0 + sg z the inverse CDF's slope sg / pdf(z) times the CDF's error
    # (relative, ~1e-15 of Phi(z)), i.e. sg Phi(z) / pdf(z) 1e-14 <= sg / |z| 1e-14 for z <= -2; plus the store
    assert np.all(err <= 1e-12 + u * np.abs(want)), float(np.max(err))
    beam = v[nf:]
    assert stats.kstest(beam, stats.truncnorm(lo, hi, loc=v0, scale=sigma).cdf).pvalue > 1e-3


def test_small_sigma_is_refused():
    """Below sigma = 1/sqrt(2 pi) the reference's density is min(pdf, 1), which the device does not draw: refused."""
    import ocplasma_amd as oc
    env = oc.BatchedPIC(1, 1000, 64, L=50.0, dt=0.05)
    try:
        for kind in ("two-stream", "bump-on-tail"):
            with pytest.raises(oc._abi.PicError):
                env.reset_sampled(kind, sigma=0.39)
            env.reset_sampled(kind, sigma=0.4)
            assert np.all(np.isfinite(env.particles()[1]))
    finally:
        env.close()
