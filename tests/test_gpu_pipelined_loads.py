"""The sweeps that store no particles (ST_A, ST_PROBE, ST_C_RO) request tile t + 1 before they push tile t (pic_sweep.h:
sweep_kernel, kAhead).  The boundaries of that loop -- a workgroup with a single tile, a last tile that only some lanes have, a
lane tail of fewer than VEC particles, a workgroup with no whole tile at all -- must give the bits of the storing schedule, whose
loop is the old one, and of the resident schedule, which has no tiles."""
import json
import os
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def oc():
    import ocplasma_amd
    return ocplasma_amd


def test_pipelined_sweeps_are_built_without_spills():
    """The second pair of tile registers leaves every sweep that uses it (stages 0, 5, 12) scratch-free and within the 64 VGPRs
    of eight waves per SIMD, for every particle format."""
    from ocplasma_amd import _build
    path = _build.RESOURCES
    if not os.path.exists(path):
        _build.build_library()
    rep = json.load(open(path))
    found = {}
    for k, v in rep.items():
        m = re.search(r"sweep_kernelINS_\d+(Pos\w\d\d)E.*Li(\d+)ELi(\d+)EEEv", k)
        if m and int(m.group(3)) in (0, 5, 12):
            found.setdefault(int(m.group(3)), set()).add(m.group(1))
            assert v["scratch_bytes_per_lane"] == 0 and v["vgprs"] <= 64, (k, v)
    assert found == {s: {"PosF64", "PosF32", "PosU32"} for s in (0, 5, 12)}, found


# a tile is 512 lanes x VEC particles: 1024 in float64, 2048 in float32; chunk = ceil(N / blocks) rounded up to tiles
CASES = [  # N, blocks_per_env, dtype, position_dtype, interpol
    (2049, 3, "float64", None, "CIC"),            # two workgroups of exactly one tile, a third with one particle (no tile, a lane tail)
    (5003, 2, "float64", None, "CIC"),            # three tiles | one tile + a partial tile + a lane tail of one particle
    (5003, 2, "float64", None, "TSC"),
    (1023, 1, "float64", None, "CIC"),            # less than one tile: some lanes have a tile, one a tail, the rest nothing
    (4099, 3, "float32", None, "CIC"),            # float32: one tile, one tile, a lane tail of three particles
    (7177, 2, "float32", None, "TSC"),            # two tiles | one tile + a partial tile + a lane tail of one particle
    (4099, 3, "float32", "fixed32", "CIC"),
    (7177, 2, "float32", "fixed32", "TSC"),
]


def _same(a, b, dtype):
    (xa, va), (xb, vb) = a.particles(), b.particles()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    for fa, fb in zip(a.fields(), b.fields()):
        assert np.array_equal(fa, fb)
    (ka, pa, ra), (kb, pb, rb) = a.energies(), b.energies()
    assert np.array_equal(pa, pb) and np.array_equal(ra, rb)
    assert np.allclose(ka, kb, rtol=1e-13 if dtype == "float64" else 1e-6)   # KE: a float64 sum in the launch geometry's order
    assert a.bad_count() == b.bad_count()


@pytest.mark.gpu
@pytest.mark.parametrize("N,bpe,dtype,pos,interpol", CASES)
def test_loop_boundaries_equal_storing_and_resident(oc, N, bpe, dtype, pos, interpol):
    L, Ng, E_ = 50.0, 128, 2
    rng = np.random.default_rng(N + bpe)
    x0 = rng.uniform(0, L, (E_, N)).astype(dtype)
    x0[x0 >= L] = 0.0
    v0 = rng.normal(0, 1.5, (E_, N)).astype(dtype)
    ext = 0.05 * rng.normal(size=(E_, Ng))
    kw = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol)
    ro = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, readonly_c="on", **kw)
    st = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, readonly_c="off", **kw)
    res = oc.BatchedPIC(E_, N, Ng, blocks_per_env=-1, **kw)
    envs = (ro, st, res)
    for env in envs:
        env.reset(x0, v0)
    # ST_PROBE: the deposit of the positions the state was reset to is the one the refresh (a storing sweep) made
    n, E, _ = ro.eval_field(x0)
    n_ref, E_ref, _ = ro.fields()
    assert np.array_equal(n, n_ref) and np.array_equal(E, E_ref)
    for env in envs:
        env.step(ext, nsteps=4)                   # first, inner and last steps of one call
        env.step(None, nsteps=1)
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    # ST_A: without the cached first deposit the step opens with a sweep that only reads; same integer sums as the cached row
    ro.invalidate()
    hs = [env.step_history(ext, 3) for env in envs]
    for h in hs[1:]:
        assert np.array_equal(hs[0][1], h[1]) and np.array_equal(hs[0][2], h[2])
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    for env in envs:
        env.close()
