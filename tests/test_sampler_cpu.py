"""The restatement of the device sampler (tests/hp_sampler.py) on its own, without a GPU: Philox4x32-10 against Random123's
known-answer vectors, u01 at its ends, the population split against the host sampler's, and the distribution it draws against
the host samplers of env/dist.py."""
from fractions import Fraction

import numpy as np
import pytest

import hp_sampler as hs


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = hs.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want
    # vectorised: the same words at every position of an array
    got = hs.philox4x32_10(*(np.full(5, c, dtype=np.uint64) for c in ctr), *key)
    assert all(np.all(g == w) for g, w in zip(got, want))


def test_u01_ends_and_the_2_52_boundary():
    # bits = 0: half a unit above zero
    assert hs.u01(0, 0) == 0.5 * 2.0 ** -53
    # bits = 2^53 - 1: (2^53 - 1) + 0.5 rounds (to even) to 2^53, so u01 returns exactly 1.0 -- (0, 1], not (0, 1)
    assert hs.u01(0xFFFFFFFF, 0xFFFFFFFF) == 1.0
    # below 2^52 bits + 0.5 is exact; from 2^52 on it rounds half to even (a multiple of 2^-52 in u)
    for bits in (2 ** 52 - 2, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 52 + 2, 2 ** 52 + 3):
        a, b = bits >> 21, (bits & ((1 << 21) - 1)) << 11
        u = Fraction(float(hs.u01(a, b)))
        exact = (Fraction(bits) + Fraction(1, 2)) / 2 ** 53
        if bits < 2 ** 52:
            assert u == exact, bits
        else:
            want = Fraction(bits + (bits & 1), 2 ** 53)      # ties to even: odd bits round up, even bits down
            assert u == want and abs(u - exact) == Fraction(1, 2 ** 54), bits
    # the low 11 bits of b never matter; every output is positive and at most 1
    assert hs.u01(123, 0x7FF) == hs.u01(123, 0)
    rng = np.random.default_rng(0)
    u = hs.u01(rng.integers(0, 2 ** 32, 10000, dtype=np.uint64), rng.integers(0, 2 ** 32, 10000, dtype=np.uint64))
    assert np.all((u > 0) & (u <= 1))


def test_population_split_matches_the_host_sampler():
    from ocplasma_amd.env.dist import BumpOnTail
    rng = np.random.default_rng(1)
    Ns = [1, 2, 3, 5, 6, 7, 10, 12, 13, 100, 999, 1000, 1001, 40000, 65537, 1 << 20, 10 ** 6 + 3]
    As = [0.0, 0.1, 0.2, 0.25, 0.3, 1 / 3, 0.5, 1.0, 3.0] + list(rng.uniform(0, 2, 20))
    for N in Ns:
        for a in As:
            s = BumpOnTail.__new__(BumpOnTail)           # the split alone, without drawing N samples
            s.a, s.n_samples = float(a), N
            high = s.inject_high_electron_indice()
            nf = hs.n_first(1, N, float(a))
            assert high.size == N - nf and (high.size == 0 or high[0] == nf), (N, a)
        assert hs.n_first(0, N, 0.0) == N // 2


def test_key_layout():
    # the two seeds differ only in their high words: the same k0, different k1
    assert hs.key(5, 0) == (5 ^ 0x85EBCA6B, 0)
    assert hs.key(5 + (7 << 32), 0) == (5 ^ 0x85EBCA6B, 7)
    assert hs.key(0, 2) == ((3 * 0x85EBCA6B) & 0xFFFFFFFF, 0)
    assert hs.key(2 ** 64 - 1, 0xFFFFFFFF) == (0xFFFFFFFF, 0xFFFFFFFF)       # env + 1 wraps to 0


def test_restatement_against_longdouble_twin():
    """The float64 restatement (NumPy's log / sqrt / cos) and the longdouble twin take the same decisions away from the edges
    and agree within velocity_bound; x does not depend on the twin."""
    for kind, v0, sigma, A in ((0, 3.0, 1.0, 0.1), (1, 4.0, 0.5, 0.05), (1, 12.0, 1.0, 0.0)):
        f = hs.sample(20000, 50.0, kind, 0.2, v0, sigma, A, 2, 11, 3)
        t = hs.sample(20000, 50.0, kind, 0.2, v0, sigma, A, 2, 11, 3, ld=True)
        assert np.array_equal(f["x"], t["x"])
        amb = hs.decisions_near_edge(t)
        ok = ~amb & (t["attempt"] <= hs.ATTEMPTS)
        assert np.array_equal(f["attempt"][ok], t["attempt"][ok])
        err = np.abs(f["v"][ok] - t["v"][ok].astype(np.float64))
        # NumPy's cos(pi ang) rounds its argument first (the device's sincospi does not): |d angle| <= 2 pi u64, times
        # sg r <= sg sqrt(-2 log 2^-54) < 9 sg
        extra = 9 * t["sg"] * 2 * np.pi * hs.U64 * (1 + A)
        assert np.all(err <= hs.velocity_bound(t, A, "float64")[ok] + extra[ok]), float(np.max(err))


@pytest.mark.parametrize("kind", ["two-stream", "bump-on-tail"])
def test_restatement_distribution_matches_host_samplers(kind):
    """KS tests of the restatement's populations (A = 0) against the host samplers' (the reference's rejection sampler)."""
    from scipy import stats
    from ocplasma_amd.env.dist import BumpOnTail, TwoStream
    N, L = 20000, 50.0
    np.random.seed(5)
    if kind == "two-stream":
        host = TwoStream(v0=3.0, sigma=1.0, n_samples=N, L=L)
        out = hs.sample(N, L, 0, 0.0, 3.0, 1.0, 0.0, 2, 17, 0)
        split = N // 2
    else:
        host = BumpOnTail(a=0.2, v0=4.0, sigma=0.5, n_samples=N, L=L)
        out = hs.sample(N, L, 1, 0.2, 4.0, 0.5, 0.0, 2, 17, 0)
        split = hs.n_first(1, N, 0.2)
    x, v = host.get_sample()
    for part in (slice(0, split), slice(split, N)):
        assert stats.ks_2samp(out["v"][part], v[part]).pvalue > 1e-3, (kind, part)
        assert stats.ks_2samp(out["xs"][part], x[part]).pvalue > 1e-3, (kind, part)
    assert np.all(np.abs(out["v_raw"]) <= hs.VMAX)
