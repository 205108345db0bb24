"""Whole steps without sweep C's stores (pic_set_readonly_c): sweep C_RO stores no particles and sweep D_RC / D2_RC
re-derives C's output from C's input and C's field tile.  Forced on, the streaming schedule must give the bits of the storing
schedule and of the resident one -- particles, fields, energies, bad-position counts -- for every particle format, shape and
stepping entry point; and the wave-uniform fast path of the wrap must leave edge positions where the reference puts them."""
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


def test_readonly_sweeps_are_built_without_spills():
    """The three new sweep stages (ST_C_RO = 12, ST_D_RC = 13, ST_D2_RC = 14) are in the library's resource report for every
    particle format, scratch-free and within the 64 VGPRs of eight waves per SIMD."""
    from ocplasma_amd import _build
    path = _build.RESOURCES
    if not os.path.exists(path):
        _build.build_library()
    rep = json.load(open(path))
    found = {}
    for k, v in rep.items():
        m = re.search(r"sweep_kernelINS_\d+(Pos\w\d\d)E.*Li(\d+)ELi(\d+)EEEv", k)
        if m and int(m.group(3)) in (12, 13, 14):
            found.setdefault(int(m.group(3)), set()).add(m.group(1))
            assert v["scratch_bytes_per_lane"] == 0 and v["vgprs"] <= 64, (k, v)
    assert found == {s: {"PosF64", "PosF32", "PosU32"} for s in (12, 13, 14)}, found


CASES = [  # N, Ng, envs, dtype, position_dtype, interpol
    (5000, 250, 3, "float64", None, "CIC"),
    (5000, 250, 3, "float64", None, "TSC"),
    (4000, 128, 2, "float32", None, "CIC"),
    (4000, 128, 2, "float32", None, "TSC"),
    (5000, 250, 3, "float32", "fixed32", "CIC"),
    (3000, 200, 2, "float32", "fixed32", "TSC"),
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
@pytest.mark.parametrize("N,Ng,E_,dtype,pos,interpol", CASES)
def test_readonly_equals_resident_and_storing(oc, N, Ng, E_, dtype, pos, interpol):
    L, M = 50.0, 3
    rng = np.random.default_rng(N + Ng + E_)
    x0 = rng.uniform(0, L, (E_, N)).astype(dtype)
    x0[x0 >= L] = 0.0
    v0 = rng.normal(0, 1.5, (E_, N)).astype(dtype)
    ext = 0.05 * rng.normal(size=(E_, Ng))
    kw = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol)
    ro = oc.BatchedPIC(E_, N, Ng, blocks_per_env=3, readonly_c="on", **kw)
    st = oc.BatchedPIC(E_, N, Ng, blocks_per_env=3, readonly_c="off", **kw)
    res = oc.BatchedPIC(E_, N, Ng, blocks_per_env=-1, **kw)
    envs = (ro, st, res)
    act = oc.E_field(L, Ng, M)
    for env in envs:
        env.set_actuator(act)
        env.reset(x0, v0)
    for env in envs:
        env.step(ext, nsteps=5)              # first, inner and last steps of one call
        env.step(None, nsteps=1)
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    hs = [env.step_history(ext, 4) for env in envs]
    for h in hs[1:]:
        assert np.array_equal(hs[0][1], h[1]) and np.array_equal(hs[0][2], h[2])
    a = rng.uniform(-1.0, 1.0, (E_, 2 * M))
    for env in envs:
        env.step_actions(a, nsteps=3)
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    traj = rng.uniform(-1.0, 1.0, (4, E_, 2 * M))
    for env in envs:
        env.step_actions_traj(traj)
        env.step_feedback(3)
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    # a staged step between whole ones keeps the storing sweep C (its caller may read the particles between the stages)
    for env in envs:
        for stage in (1, 2):
            env._h.step_stage(stage, ext)
    assert np.array_equal(ro.particles()[0], st.particles()[0])
    for env in envs:
        env._h.step_stage(3, ext)
        env.step(ext, nsteps=2)
    _same(ro, st, dtype)
    _same(ro, res, dtype)
    for env in envs:
        env.close()


@pytest.mark.gpu
def test_readonly_golden_trajectory(oc):
    """The reference's 500-step two-stream trajectory (g5) on the streaming schedule with the read-only sweep C forced on."""
    g = load_golden("g5_two_stream_N5000_Ng250")
    L, Ng = float(g["L"]), int(g["Ng"])
    env = oc.BatchedPIC(1, int(g["N"]), Ng, L=L, dt=float(g["dt_in"]), blocks_per_env=2, readonly_c="on")
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
def test_readonly_config2_size_equals_storing(oc):
    """Config 2's shape (64 environments of 1e6, Ng = 256, float64): the automatic choice is on there, and 20 steps in one call
    with it forced on and off give the same bits."""
    E_, N, Ng, L = 64, 1_000_000, 256, 50.0
    envs = [oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, readonly_c=m) for m in ("on", "off")]
    for env in envs:
        env.reset_sampled("bump-on-tail", seed=11)
        env.step(None, nsteps=20)
    _same(envs[0], envs[1], "float64")
    assert envs[0].bad_count() == 0
    for env in envs:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("interpol", ["CIC", "TSC"])
def test_readonly_edge_positions(oc, po, interpol):
    """Positions at and next to the box edges (0, -0.0, L - ulp, and velocities that carry particles across 0 and L within a
    sub-stage) go through the sweeps with the fast wrap as the oracle steps them; non-finite ones are counted the same way
    whether sweep C stores or not."""
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
    envs = [oc.BatchedPIC(1, N, Ng, L=L, dt=0.1, interpol=interpol, blocks_per_env=1, readonly_c=m) for m in ("on", "off")]
    for env in envs:
        env.reset(x[None], v[None])
        env.step(None, nsteps=3)
    _same(envs[0], envs[1], "float64")
    ref = po.OraclePIC(x.copy(), v.copy(), Ng, L=L, dt=envs[0].dt, perturb=False, faithful=False, interpol=interpol)
    for _ in range(3):
        ref.update_state(np.zeros((Ng, 1)))
    xg, vg = envs[0].particles()
    assert circ_err(xg[0], ref.x, L) / L < 1e-12 and rel_err(vg[0], ref.v) < 1e-12
    assert np.all((xg[0] >= 0) & (xg[0] < L)) and not np.any(np.signbit(xg[0]))
    assert envs[0].bad_count() == 0
    # non-finite positions: counted and parked, identically with and without the stores
    x2 = x.copy()
    x2[300], x2[301], x2[302] = np.inf, -np.inf, np.nan
    for env in envs:
        env.reset(x2[None], v[None])
        env.step(None, nsteps=2)
    _same(envs[0], envs[1], "float64")
    assert envs[0].bad_count() > 0
    for env in envs:
        env.close()
