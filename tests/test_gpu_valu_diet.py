"""The read-only sweeps shed VALU work their result does not need (pic_sweep.h, pic_device.h):

* the whole tiles of a workgroup's chunk whose successor is a whole tile too run in a wave-uniform loop, two tiles per trip; the
  last whole tile, the partial tile and the lane tail stay with the per-lane loop;
* `to_fixed` subtracts the high words of the two bit patterns alone (the low word of the magic constant is zero);
* a CIC `locate` behind a wrap does not fold the index Ng to node 0 in the sweeps: slots Ng and Ng + 1 of their LDS meshes and
  field tiles stand for nodes 0 and 1.

Bits, not tolerances: against the storing schedule, against the resident schedule (which has no tiles and still folds) and
against an integer-exact NumPy restatement of the oracle's deposit.  KE alone is a float64 sum in the launch geometry's order --
and so are the LDS sums of `accum_dtype="float64"`, whose case asserts bits where a single wave deposits and a derived bound
elsewhere (test_index_ng_with_float64_accumulators)."""
import json
import os
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def oc():
    import ocplasma_amd
    return ocplasma_amd


@pytest.fixture(scope="module")
def po():
    from oracle import pic_oracle
    return pic_oracle


def _fg(N):
    """Fractional bits of the fixed-point accumulators (host_plan.h: the weights of all N particles on one node fit in 63 bits)."""
    lg = 0
    while (1 << lg) < N + 1:
        lg += 1
    return min(50, 62 - lg)


def _exact_density(x, N, Ng, L, n0=1.0):
    """The oracle's CIC deposit (oracle/pic_oracle.py: cic -- same wrap, same cell, same weight expressions) with the sums made
    exact: every weight rounded to 2^-fg (nearest, ties to even: what adding 1.5 2^(52 - fg) does) and summed as an integer, as
    the device's accumulators do.  An index the division rounds up to Ng goes to nodes 0 and 1 with the weights of the unfolded
    index (the reference itself raises there: bincount grows a bin)."""
    dx = L / Ng
    fg = _fg(N)
    xw = np.mod(np.mod(x, L), L)
    jl = np.floor(xw / dx).astype(np.int64)
    jr = jl + 1
    wl = (jr * dx - xw) / dx
    wr = (xw - jl * dx) / dx
    il = np.rint(wl * 2.0 ** fg).astype(np.int64)
    ir = np.rint(wr * 2.0 ** fg).astype(np.int64)
    acc = np.zeros(Ng, np.int64)
    np.add.at(acc, np.mod(jl, Ng), il)
    np.add.at(acc, np.mod(jr, Ng), ir)
    return (acc.astype(np.float64) * 2.0 ** -fg) * (n0 * L / N / dx)      # interpolate.py:18, left to right


# ---------------------------------------------------------------------------------------------------------------------
# 3. to_fixed: the word identity, on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_to_fixed_high_word_identity():
    """bits(w + magic) - bits(magic) == (hi32(bits(w + magic)) - hi32(bits(magic)), lo32(bits(w + magic))) for every fg the host
    chooses, negative differences included, because lo32(bits(magic)) == 0."""
    for fg in range(38, 51):
        magic = np.float64(1.5 * 2.0 ** (52 - fg))
        mbits = magic.view(np.uint64)
        assert int(mbits) & 0xFFFFFFFF == 0, fg
        u = 2.0 ** -(fg + 1)
        rng = np.random.default_rng(fg)
        w = np.concatenate([[0.0, 1.0, u, -u, 3 * u, -3 * u, 5 * u, -1e-300, -2.0 ** -60, -2.0 ** -(fg + 2), 1 + 2.0 ** -40,
                             2.0 ** -fg, -2.0 ** -fg, 1 - 2.0 ** -fg], rng.uniform(0, 1, 4000), -rng.uniform(0, 1e-6, 500)])
        s = (w + magic).view(np.uint64)
        full = (s - mbits).view(np.int64)                                  # 64-bit subtraction, modulo 2^64
        hi = ((s >> np.uint64(32)).astype(np.uint32) - np.uint32(int(mbits) >> 32)).astype(np.uint64)     # modulo 2^32
        words = ((hi << np.uint64(32)) | (s & np.uint64(0xFFFFFFFF))).view(np.int64)
        assert np.array_equal(full, words), fg
        # and it IS round-to-nearest-even of w 2^fg
        assert np.array_equal(full, np.rint(w * 2.0 ** fg).astype(np.int64)), fg


# ---------------------------------------------------------------------------------------------------------------------
# 4. resources
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_sweeps_keep_their_registers():
    """Stages 0, 5 and 12 of all three formats: no scratch, at most 64 VGPRs; float64 C_RO keeps seven waves per SIMD."""
    from ocplasma_amd import _build
    path = _build.RESOURCES
    if not os.path.exists(path):
        _build.build_library()
    rep = json.load(open(path))
    found, c_ro_f64 = {}, []
    for k, v in rep.items():
        m = re.search(r"sweep_kernelINS_\d+(Pos\w\d\d)E.*Li(\d+)ELi(\d+)EEEv", k)
        if m and int(m.group(3)) in (0, 5, 12):
            found.setdefault(int(m.group(3)), set()).add(m.group(1))
            assert v["scratch_bytes_per_lane"] == 0 and v["vgprs"] <= 64, (k, v)
            if int(m.group(3)) == 12 and m.group(1) == "PosF64":
                c_ro_f64.append(k)
                assert v["waves_per_simd"] >= 7, (k, v)
    assert found == {s: {"PosF64", "PosF32", "PosU32"} for s in (0, 5, 12)}, found
    assert c_ro_f64


# ---------------------------------------------------------------------------------------------------------------------
# 1. loop boundaries
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b, dtype):
    (xa, va), (xb, vb) = a.particles(), b.particles()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    for fa, fb in zip(a.fields(), b.fields()):
        assert np.array_equal(fa, fb)
    (ka, pa, ra), (kb, pb, rb) = a.energies(), b.energies()
    assert np.array_equal(pa, pb) and np.array_equal(ra, rb)
    assert np.allclose(ka, kb, rtol=1e-13 if dtype == "float64" else 1e-6, atol=0)   # KE: a float64 sum in the launch geometry's order
    assert a.bad_count() == b.bad_count()


# A tile is 512 lanes x VEC particles: 1024 in float64, 2048 in float32 and fixed32; chunk = ceil(N / blocks) rounded up to tiles.
# nfull = whole tiles of a workgroup; the uniform loop runs nfull - 1 tiles (none below nfull = 2), two per trip and an odd one.
CASES = [  # N, blocks_per_env, dtype, position_dtype, interpol
    (1024, 1, "float64", None, "CIC"),            # nfull = 1, nothing behind it
    (2048, 1, "float64", None, "CIC"),            # nfull = 2: one uniform tile (the odd one), nothing behind the last whole tile
    (2049, 1, "float64", None, "CIC"),            # ... and a lane tail of one particle
    (3072, 1, "float64", None, "CIC"),            # nfull = 3: one two-tile trip
    (3073, 1, "float64", None, "CIC"),
    (4607, 1, "float64", None, "CIC"),            # nfull = 4: a trip and the odd one; a partial tile and a lane tail
    (5121, 1, "float64", None, "CIC"),            # nfull = 5: two trips
    (6144, 1, "float64", None, "CIC"),            # nfull = 6: two trips and the odd one, nothing behind
    (5003, 2, "float64", None, "CIC"),            # nfull = 3 | 1 + a partial tile + a lane tail
    (6145, 3, "float64", None, "CIC"),            # nfull = 3 | 3 | 0 (one particle)
    (900, 1, "float64", None, "CIC"),             # nfull = 0: a partial tile alone
    (5003, 2, "float64", None, "TSC"),
    (6145, 1, "float64", None, "TSC"),            # nfull = 6 and a lane tail
    (4096, 1, "float32", None, "CIC"),            # float32: nfull = 2
    (6147, 1, "float32", None, "CIC"),            # nfull = 3 and a lane tail of three
    (10241, 1, "float32", None, "TSC"),           # nfull = 5
    (10006, 2, "float32", None, "CIC"),           # nfull = 3 | 1 + partial + tail
    (4096, 1, "float32", "fixed32", "CIC"),
    (6147, 1, "float32", "fixed32", "TSC"),
    (10241, 1, "float32", "fixed32", "CIC"),
    (12290, 3, "float32", "fixed32", "CIC"),      # nfull = 3 | 3 | 0 (two particles)
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,bpe,dtype,pos,interpol", CASES)
def test_uniform_loop_boundaries_equal_storing_and_resident(oc, N, bpe, dtype, pos, interpol):
    L, Ng, E_ = 50.0, 128, 2
    rng = np.random.default_rng(N + bpe)
    x0 = rng.uniform(0, L, (E_, N)).astype(dtype)
    x0[x0 >= L] = 0.0
    v0 = rng.normal(0, 1.5, (E_, N)).astype(dtype)
    ext = 0.05 * rng.normal(size=(E_, Ng))
    kw = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol)
    ro = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, readonly_c="on", **kw)
    st = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, readonly_c="off", **kw)
    # (the resident schedule holds at most 8192 particles per environment: the float32 shapes with five tiles go without it)
    envs = (ro, st) + ((oc.BatchedPIC(E_, N, Ng, blocks_per_env=-1, **kw),) if N <= 8192 else ())
    for env in envs:
        env.reset(x0, v0)
    # ST_PROBE: the deposit of the positions the state was reset to is the one the refresh (a storing sweep) made
    n, E, _ = ro.eval_field(x0)
    n_ref, E_ref, _ = ro.fields()
    assert np.array_equal(n, n_ref) and np.array_equal(E, E_ref)
    for env in envs:
        env.step(ext, nsteps=4)                   # first, inner and last steps of one call
        env.step(None, nsteps=1)
    for other in envs[1:]:
        _same(ro, other, dtype)
    # ST_A: without the cached first deposit the step opens with a sweep that only reads; same integer sums as the cached row
    ro.invalidate()
    hs = [env.step_history(ext, 3) for env in envs]
    for h in hs[1:]:
        assert np.array_equal(hs[0][1], h[1]) and np.array_equal(hs[0][2], h[2])
    for other in envs[1:]:
        _same(ro, other, dtype)
    for env in envs:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. j == Ng
# ---------------------------------------------------------------------------------------------------------------------
def _edge_state(Ng, N, L, dtype="float64", seed=0):
    """Random particles, and a few hundred at nextafter(L, 0), at 0 and at the two values next to each, at rest."""
    rng = np.random.default_rng(Ng + seed)
    T = np.dtype(dtype).type
    x = rng.uniform(0, L, N).astype(dtype)
    x[x >= T(L)] = 0
    v = rng.normal(0, 1.0, N).astype(dtype)
    top = np.nextafter(T(L), T(0))
    edge = [top, np.nextafter(top, T(0)), T(L), T(0), np.nextafter(T(0), T(1)), -np.nextafter(T(0), T(1))]
    idx = rng.permutation(N)[:360]
    for m, e in enumerate(edge):
        x[idx[m::len(edge)]] = e
    v[idx] = 0
    return x, v


@pytest.mark.gpu
@pytest.mark.parametrize("Ng", [150, 300])
def test_index_ng_is_deposited_and_gathered_as_node_0(oc, Ng):
    L, N = 50.0, 3001
    dx = L / Ng
    if np.floor(np.nextafter(L, 0.0) / dx) != Ng:
        pytest.skip(f"floor(nextafter(L, 0) / dx) != Ng at Ng = {Ng}")
    x, v = _edge_state(Ng, N, L)
    assert np.count_nonzero(np.floor(np.mod(np.mod(x, L), L) / dx) == Ng) >= 50
    want = _exact_density(x, N, Ng, L)
    x0, v0 = np.stack([x, x[::-1]]), np.stack([v, v[::-1]])
    for bpe in (1, 2):
        kw = dict(L=L, dt=0.1, blocks_per_env=bpe)
        ro = oc.BatchedPIC(2, N, Ng, readonly_c="on", **kw)
        st = oc.BatchedPIC(2, N, Ng, readonly_c="off", **kw)
        res = oc.BatchedPIC(2, N, Ng, L=L, dt=0.1, blocks_per_env=-1)
        for env in (ro, st, res):
            env.reset(x0, v0)
            n = env.fields()[0]
            assert np.array_equal(n[0], want) and np.array_equal(n[1], want)      # REFRESH / the resident kernel's deposit
        n, E, _ = ro.eval_field(x0)                                               # PROBE
        assert np.array_equal(n[0], want) and np.array_equal(n[1], want)
        assert np.array_equal(E, ro.fields()[1])
        for env in (ro, st, res):
            env.step(None, nsteps=3)
        _same(ro, st, "float64")
        _same(ro, res, "float64")                  # the resident kernel folds the index: other code, same bits
        ro.invalidate()                            # sweep A
        for env in (ro, st, res):
            env.step(None, nsteps=1)
        _same(ro, st, "float64")
        _same(ro, res, "float64")
        assert ro.bad_count() == 0
        for env in (ro, st, res):
            env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("Ng", [150, 300])
def test_index_ng_with_float64_accumulators(oc, Ng):
    """ds_add_f64 sums depend on the order in which the waves' atomics land, so bits can be asked only where one wave deposits:
    N = 128 is lanes 0..63 of one workgroup, whose atomics on one LDS word are served in lane order.  At N = 3001 the two
    schedules and the integer accumulators agree to the rounding of those sums: a node holds at most N weights in [0, 1], a
    float64 sum of them is off by at most N 2^-53 of itself (3.3e-13), and the field by L times that at the most, 2e-11; three
    steps at dt = 0.1 move no particle by more (bound asserted: 1e-10).  A deposit on the wrong node would shift the density by Ng / N of its mean."""
    L = 50.0
    dx = L / Ng
    if np.floor(np.nextafter(L, 0.0) / dx) != Ng:
        pytest.skip(f"floor(nextafter(L, 0) / dx) != Ng at Ng = {Ng}")
    for N, exact in ((128, True), (3001, False)):
        x, v = _edge_state(Ng, N, L, seed=N)
        if N == 128:
            x[:24] = np.nextafter(L, 0.0)
            v[:24] = 0
        x0, v0 = x[None], v[None]
        want = _exact_density(x, N, Ng, L)
        kw = dict(L=L, dt=0.1, blocks_per_env=1)
        ro = oc.BatchedPIC(1, N, Ng, readonly_c="on", accum_dtype="float64", **kw)
        st = oc.BatchedPIC(1, N, Ng, readonly_c="off", accum_dtype="float64", **kw)
        fx = oc.BatchedPIC(1, N, Ng, readonly_c="on", **kw)
        for env in (ro, st, fx):
            env.reset(x0, v0)
        for env in (ro, st):
            # (float64 sums of float64 weights against integer sums of weights rounded to 2^-50, times Ng / N <= 2.4: at most
            # N (2^-51 + 2^-53) 2.4 = 4e-12 on a node that held every particle)
            assert np.allclose(env.fields()[0][0], want, rtol=0, atol=1e-11)
            assert np.allclose(env.eval_field(x0)[0][0], want, rtol=0, atol=1e-11)
        for env in (ro, st, fx):
            env.step(None, nsteps=3)
        if exact:
            _same(ro, st, "float64")
        for other in (st, fx):
            (xa, va), (xb, vb) = ro.particles(), other.particles()
            d = np.abs(xa - xb)
            print(f"Ng={Ng} N={N}: max|dx|={np.max(np.minimum(d, L - d)):.2e} max|dv|={np.max(np.abs(va - vb)):.2e} "
                  f"max|dE|={np.max(np.abs(ro.fields()[1] - other.fields()[1])):.2e}")
            assert np.max(np.minimum(d, L - d)) < 1e-10 and np.max(np.abs(va - vb)) < 1e-10
            assert np.allclose(ro.fields()[0], other.fields()[0], rtol=0, atol=1e-8)   # (positions 1e-10 apart: weights 1e-10 / dx apart)
            assert np.max(np.abs(ro.fields()[1] - other.fields()[1])) < 1e-10
        assert ro.bad_count() == 0
        for env in (ro, st, fx):
            env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("Ng", [150, 300])
@pytest.mark.parametrize("dtype,pos,interpol", [("float64", None, "TSC"), ("float32", None, "TSC"), ("float32", "fixed32", "CIC"),
                                                ("float32", None, "CIC")])
def test_paths_that_keep_the_fold_are_unchanged(oc, Ng, dtype, pos, interpol):
    """TSC, fixed-point positions and the packed accumulator (float32 CIC) keep the fold: their schedules still agree in bits at
    the same edge positions."""
    L, N = 50.0, 3001
    x, v = _edge_state(Ng, N, L, dtype)
    x0, v0 = np.stack([x, x[::-1]]), np.stack([v, v[::-1]])
    kw = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol)
    ro = oc.BatchedPIC(2, N, Ng, blocks_per_env=2, readonly_c="on", **kw)
    st = oc.BatchedPIC(2, N, Ng, blocks_per_env=2, readonly_c="off", **kw)
    res = oc.BatchedPIC(2, N, Ng, blocks_per_env=-1, **kw)
    for env in (ro, st, res):
        env.reset(x0, v0)
    n, E, _ = ro.eval_field(x0)
    for env in (ro, st, res):
        assert np.array_equal(env.fields()[0], n) and np.array_equal(env.fields()[1], E)
        env.step(None, nsteps=3)
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    for env in (ro, st, res):
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. to_fixed on the device: the largest sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_largest_sums_equal_the_oracle(oc, po):
    """N = 2^17 + 1 particles in one cell put every weight on two nodes.  With Ng = 128, dx = 25/64 is exact and so are the
    weights 3/4 and 1/4 of a particle a quarter into its cell: the oracle's own float64 sums are exact and must be met bit for
    bit.  With the particles spread over the cell the sums are compared with the oracle's weights summed as integers."""
    L, Ng, N = 50.0, 128, 2 ** 17 + 1
    dx = L / Ng
    rng = np.random.default_rng(17)
    quarter = np.full(N, 77.25 * dx)
    spread = (77 + rng.uniform(0, 1, N)) * dx
    spread[:3] = [77 * dx, np.nextafter(78 * dx, 0), 77.5 * dx]
    env = oc.BatchedPIC(2, N, Ng, L=L, dt=0.1)
    x0 = np.stack([quarter, spread])
    env.reset(x0, np.zeros_like(x0))
    n = env.fields()[0]
    n_or = po.density(quarter.reshape(-1, 1).copy(), dx, Ng, 1.0, L, N)[0]
    assert n_or[77] == 0.75 * N * (L / N / dx) and np.count_nonzero(n_or) == 2
    assert np.array_equal(n[0], n_or)
    assert np.array_equal(n[0], _exact_density(quarter, N, Ng, L))
    assert np.array_equal(n[1], _exact_density(spread, N, Ng, L))
    n_p = env.eval_field(x0)[0]                                      # PROBE
    assert np.array_equal(n_p, n)
    env.close()
