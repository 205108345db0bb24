"""Particles stored in every other sweep (pic_set_alternate_stores): inside a call of whole Yoshida-4 steps every
second inner step runs B2_RO, C_RB, D2_RO -- one storing sweep, which re-derives sweep B -- and the step behind it opens with
B2_RD, which re-derives sweep D.  Forced on, the mode must give the bits of the storing schedule and of the resident one --
particles, fields, energies, history rows, bad-position counts -- for every particle format, shape, call length and stepping entry
point.  KE alone is a float64 sum in the launch geometry's order, and so are the LDS sums of `accum_dtype="float64"`."""
import json
import os
import re

import numpy as np
import pytest

from conftest import circ_err, load_golden, rel_err


@pytest.fixture(scope="module")
def oc():
    import ocplasma_amd
    return ocplasma_amd


@pytest.fixture(scope="module")
def po():
    from oracle import pic_oracle
    return pic_oracle


ALT = dict(readonly_c="on", alternate_stores="on")


def test_alternate_sweeps_are_built_without_spills():
    """The four new sweep stages (ST_B2_RO = 15, ST_C_RB = 16, ST_D2_RO = 17, ST_B2_RD = 18) are in the library's resource report
    for every particle format, scratch-free and within the 64 VGPRs of eight waves per SIMD."""
    from ocplasma_amd import _build
    path = _build.RESOURCES
    if not os.path.exists(path):
        _build.build_library()
    rep = json.load(open(path))
    found = {}
    for k, v in rep.items():
        m = re.search(r"sweep_kernelINS_\d+(Pos\w\d\d)E.*Li(\d+)ELi(\d+)EEEv", k)
        if m and int(m.group(3)) in (15, 16, 17, 18):
            found.setdefault(int(m.group(3)), set()).add(m.group(1))
            assert v["scratch_bytes_per_lane"] == 0 and v["vgprs"] <= 64, (k, v)
    assert found == {s: {"PosF64", "PosF32", "PosU32"} for s in (15, 16, 17, 18)}, found


def test_python_surface_rejects_unknown_mode(oc):
    with pytest.raises(ValueError):
        oc.BatchedPIC(1, 100, 16, alternate_stores="sometimes")


def _same(a, b, dtype):
    (xa, va), (xb, vb) = a.particles(), b.particles()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    for fa, fb in zip(a.fields(), b.fields()):
        assert np.array_equal(fa, fb)
    (ka, pa, ra), (kb, pb, rb) = a.energies(), b.energies()
    assert np.array_equal(pa, pb) and np.array_equal(ra, rb)
    assert np.allclose(ka, kb, rtol=1e-13 if dtype == "float64" else 1e-6, atol=0)   # KE: a float64 sum in the launch geometry's order
    assert a.bad_count() == b.bad_count()


def _same_hist(hs, dtype):
    for h in hs[1:]:
        assert np.allclose(hs[0][0], h[0], rtol=1e-13 if dtype == "float64" else 1e-6, atol=0)
        assert np.array_equal(hs[0][1], h[1]) and np.array_equal(hs[0][2], h[2])


CASES = [  # N, Ng, envs, dtype, position_dtype, interpol, blocks_per_env  (tests/test_gpu_readonly_c.py's six formats)
    (5000, 250, 3, "float64", None, "CIC", 3),
    (5000, 250, 3, "float64", None, "TSC", 1),
    (4000, 128, 2, "float32", None, "CIC", 1),
    (4000, 128, 2, "float32", None, "TSC", 3),
    (5000, 250, 3, "float32", "fixed32", "CIC", 3),
    (3000, 200, 2, "float32", "fixed32", "TSC", 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,Ng,E_,dtype,pos,interpol,bpe", CASES)
def test_alternate_equals_resident_and_storing(oc, N, Ng, E_, dtype, pos, interpol, bpe):
    L, M = 50.0, 3
    rng = np.random.default_rng(N + Ng + E_ + bpe)
    x0 = rng.uniform(0, L, (E_, N)).astype(dtype)
    x0[x0 >= L] = 0.0
    v0 = rng.normal(0, 1.5, (E_, N)).astype(dtype)
    ext = 0.05 * rng.normal(size=(E_, Ng))
    kw = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol)
    alt = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, **ALT, **kw)
    st = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, readonly_c="off", **kw)
    res = oc.BatchedPIC(E_, N, Ng, blocks_per_env=-1, **kw)
    envs = (alt, st, res)
    act = oc.E_field(L, Ng, M)
    for env in envs:
        env.set_actuator(act)
        env.reset(x0, v0)
    for K in range(1, 7):                        # both parities; K = 1 and 2 have no step that stores once
        for env in envs:
            env.step(ext if K % 2 else None, nsteps=K)
        _same(alt, st, dtype)
        _same(alt, res, dtype)
    _same_hist([env.step_history(ext, 5) for env in envs], dtype)
    _same(alt, st, dtype)
    a = rng.uniform(-1.0, 1.0, (E_, 2 * M))
    for env in envs:
        env.step_actions(a, nsteps=4)
    _same(alt, st, dtype)
    _same(alt, res, dtype)
    traj = rng.uniform(-1.0, 1.0, (5, E_, 2 * M))
    for env in envs:
        env.step_actions_traj(traj)
        env.step_feedback(3)                     # (the feedback law needs each step's field: the call falls back)
    _same(alt, st, dtype)
    _same(alt, res, dtype)
    # a staged step between two whole-step calls, and a call of 3 right after a call of 4
    for env in envs:
        env.step(ext, nsteps=4)
        for stage in (1, 2):
            env._h.step_stage(stage, ext)
    assert np.array_equal(alt.particles()[0], st.particles()[0])
    for env in envs:
        env._h.step_stage(3, ext)
        env.step(ext, nsteps=4)
        env.step(None, nsteps=3)
    _same(alt, st, dtype)
    _same(alt, res, dtype)
    for env in envs:
        env.close()


# A tile is 512 lanes x VEC particles: 1024 in float64, 2048 in float32 and fixed32; chunk = ceil(N / blocks) rounded up to tiles.
# nfull = whole tiles of a workgroup; the uniform loop of the sweeps that store nothing runs nfull - 1 tiles (none below nfull = 2),
# two per trip and an odd one (tests/test_gpu_valu_diet.py).
LOOP_CASES = [  # N, blocks_per_env, dtype, position_dtype, interpol
    (900, 1, "float64", None, "CIC"),             # nfull = 0: a partial tile alone
    (1024, 1, "float64", None, "CIC"),            # nfull = 1, nothing behind it
    (2048, 1, "float64", None, "CIC"),            # nfull = 2: one uniform tile (the odd one)
    (2049, 1, "float64", None, "CIC"),            # ... and a lane tail of one particle
    (3073, 1, "float64", None, "CIC"),            # nfull = 3: one two-tile trip
    (4607, 1, "float64", None, "CIC"),            # nfull = 4: a trip and the odd one; a partial tile and a lane tail
    (5003, 2, "float64", None, "CIC"),            # nfull = 3 | 1 + a partial tile + a lane tail
    (6145, 3, "float64", None, "CIC"),            # nfull = 3 | 3 | 0 (one particle)
    (5003, 2, "float64", None, "TSC"),
    (4096, 1, "float32", None, "CIC"),            # float32: nfull = 2
    (6147, 1, "float32", None, "CIC"),            # nfull = 3 and a lane tail of three
    (8193, 1, "float32", None, "TSC"),            # nfull = 4
    (10006, 2, "float32", None, "CIC"),           # nfull = 3 | 1 + partial + tail
    (4096, 1, "float32", "fixed32", "CIC"),
    (6147, 1, "float32", "fixed32", "TSC"),
    (8193, 1, "float32", "fixed32", "CIC"),
    (12290, 3, "float32", "fixed32", "CIC"),      # nfull = 3 | 3 | 0 (two particles)
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,bpe,dtype,pos,interpol", LOOP_CASES)
def test_loop_boundaries_equal_storing_and_resident(oc, N, bpe, dtype, pos, interpol):
    L, Ng, E_ = 50.0, 128, 2
    rng = np.random.default_rng(N + bpe)
    x0 = rng.uniform(0, L, (E_, N)).astype(dtype)
    x0[x0 >= L] = 0.0
    v0 = rng.normal(0, 1.5, (E_, N)).astype(dtype)
    ext = 0.05 * rng.normal(size=(E_, Ng))
    kw = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol)
    alt = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, **ALT, **kw)
    st = oc.BatchedPIC(E_, N, Ng, blocks_per_env=bpe, readonly_c="off", **kw)
    # (the resident schedule holds at most 8192 particles per environment)
    envs = (alt, st) + ((oc.BatchedPIC(E_, N, Ng, blocks_per_env=-1, **kw),) if N <= 8192 else ())
    for env in envs:
        env.reset(x0, v0)
        env.step(ext, nsteps=5)                   # X Y X Y X
        env.step(None, nsteps=4)                  # X X Y X
    for other in envs[1:]:
        _same(alt, other, dtype)
    _same_hist([env.step_history(ext, 3) for env in envs], dtype)
    for other in envs[1:]:
        _same(alt, other, dtype)
    for env in envs:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("interpol", ["CIC", "TSC"])
def test_alternate_edge_positions(oc, po, interpol):
    """tests/test_gpu_readonly_c.py's edge vector through four steps in one call (X X Y X), so that the wrap B2_RD re-derives
    sees it: the bits of the storing schedule, the oracle to that test's tolerances, x in [0, L) and no negative zero; non-finite
    positions are counted the same way."""
    L, Ng, N = 50.0, 64, 4096
    rng = np.random.default_rng(5)
    x = rng.uniform(0, L, N)
    v = rng.normal(0, 1.0, N)
    edge = np.array([0.0, -0.0, np.nextafter(L, 0.0), 1e-300, L - 1e-12, 1e-12, np.nextafter(0.0, 1.0)])
    x[:edge.size] = edge
    v[:edge.size] = [0.0, 0.0, 0.0, -1.0, 1.0, -1.0, -2.0]
    x[100:140] = np.linspace(L - 0.02, L - 1e-9, 40)          # whole waves within one drift of the edge
    v[100:140] = 0.5
    x[200:240] = np.linspace(1e-9, 0.02, 40)
    v[200:240] = -0.5
    envs = [oc.BatchedPIC(1, N, Ng, L=L, dt=0.1, interpol=interpol, blocks_per_env=1, **m)
            for m in (ALT, dict(readonly_c="off"))]
    for env in envs:
        env.reset(x[None], v[None])
        env.step(None, nsteps=4)
    _same(envs[0], envs[1], "float64")
    ref = po.OraclePIC(x.copy(), v.copy(), Ng, L=L, dt=envs[0].dt, perturb=False, faithful=False, interpol=interpol)
    for _ in range(4):
        ref.update_state(np.zeros((Ng, 1)))
    xg, vg = envs[0].particles()
    assert circ_err(xg[0], ref.x, L) / L < 1e-12 and rel_err(vg[0], ref.v) < 1e-12
    assert np.all((xg[0] >= 0) & (xg[0] < L)) and not np.any(np.signbit(xg[0]))
    assert envs[0].bad_count() == 0
    x2 = x.copy()
    x2[300], x2[301], x2[302] = np.inf, -np.inf, np.nan
    for env in envs:
        env.reset(x2[None], v[None])
        env.step(None, nsteps=4)
    _same(envs[0], envs[1], "float64")
    assert envs[0].bad_count() > 0
    for env in envs:
        env.close()


@pytest.mark.gpu
def test_alternate_golden_trajectory(oc):
    """The reference's 500-step two-stream trajectory (g5) in calls of 100 with the mode forced on, to the tolerances of
    tests/test_gpu_readonly_c.py::test_readonly_golden_trajectory."""
    g = load_golden("g5_two_stream_N5000_Ng250")
    L, Ng = float(g["L"]), int(g["Ng"])
    env = oc.BatchedPIC(1, int(g["N"]), Ng, L=L, dt=float(g["dt_in"]), blocks_per_env=2, **ALT)
    assert env._h.schedule() == "streaming"
    env.reset(g["x_init"].reshape(1, -1), g["v_init"].reshape(1, -1))
    H = []
    for k in range(5):
        ke, pe, _ = env.step_history(None, 100)
        H.extend((ke + pe)[:, 0])
        K = (k + 1) * 100
        if K in (100, 500):
            x, v = env.particles()
            tol = 1e-11 if K == 100 else 1e-7
            assert circ_err(x[0], g[f"x_{K}"], L) / L < tol and rel_err(v[0], g[f"v_{K}"]) < tol
            assert rel_err(env.fields()[1][0], g[f"E_mesh_{K}"]) < (5e-11 if K == 100 else 5e-8)
    assert rel_err(H, g["H"][1:]) < 1e-10
    env.close()


@pytest.mark.gpu
def test_alternate_launches_match_schedule(oc):
    """One launch per descriptor with the mode on: reset, step(1), step(5) and step_history(4) launch what
    tests/schedule_alt_driver.cpp prints for "0 0 1 1 i r s1 s5 s4" (tests/test_schedule_alt_cpu.py holds the driver to these
    counts): three sweeps a step, one solve a call, the refresh's sweep and solve."""
    E, N, Ng, L = 2, 3000, 64, 50.0
    env = oc.BatchedPIC(E, N, Ng, L=L, dt=0.1, blocks_per_env=2, **ALT)
    assert env._h.schedule() == "streaming"
    rng = np.random.default_rng(11)
    env.profile(True)
    env.reset(rng.uniform(0.0, L, (E, N)), rng.normal(0.0, 1.0, (E, N)))
    env.step(None, 1)
    env.step(None, 5)
    env.step_history(None, 4)
    env.sync()
    prof = {k: n for k, (_, n) in env.profile_read().items()}
    env.close()
    assert prof == {"sweep_B": 10, "sweep_C": 10, "sweep_D": 10, "field_solve": 4, "sweep_aux": 1}, prof


@pytest.mark.gpu
def test_alternate_with_float64_accumulators(oc):
    """ds_add_f64 sums depend on the order in which the waves' atomics land, so bits are asked only where one wave deposits
    (N = 128 in one workgroup).  At N = 3001 the bound is the one tests/test_gpu_valu_diet.py derives for three steps at dt = 0.1
    (a float64 sum of at most N weights is off by at most N 2^-53 of itself, the field by L times that: 2e-11; asserted 1e-10);
    three steps in one call are X Y X."""
    L, Ng = 50.0, 150
    for N, exact in ((128, True), (3001, False)):
        rng = np.random.default_rng(N)
        x0 = rng.uniform(0, L, (1, N))
        v0 = rng.normal(0, 1.0, (1, N))
        kw = dict(L=L, dt=0.1, blocks_per_env=1, accum_dtype="float64")
        alt = oc.BatchedPIC(1, N, Ng, **ALT, **kw)
        st = oc.BatchedPIC(1, N, Ng, readonly_c="off", **kw)
        for env in (alt, st):
            env.reset(x0, v0)
            env.step(None, nsteps=3)
        if exact:
            _same(alt, st, "float64")
        (xa, va), (xb, vb) = alt.particles(), st.particles()
        d = np.abs(xa - xb)
        print(f"N={N}: max|dx|={np.max(np.minimum(d, L - d)):.2e} max|dv|={np.max(np.abs(va - vb)):.2e} "
              f"max|dE|={np.max(np.abs(alt.fields()[1] - st.fields()[1])):.2e}")
        assert np.max(np.minimum(d, L - d)) < 1e-10 and np.max(np.abs(va - vb)) < 1e-10
        assert np.max(np.abs(alt.fields()[1] - st.fields()[1])) < 1e-10
        assert alt.bad_count() == 0
        for env in (alt, st):
            env.close()
