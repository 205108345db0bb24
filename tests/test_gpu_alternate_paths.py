"""The alternate stores (pic_set_alternate_stores) on the paths a production-sized state takes and no small test
did: calls that the recorder or an open tape cuts into parts, the tape's replay, adjoint and forward mode over a forward made of
re-derived sub-stages, per-step fields, a first step that has to deposit q1 itself, single-step parts under the read-only sweep
C, and the calls on which the mode must not engage.  Forced on, every one of them must give the bits of the storing schedule
(and of the resident one where it applies): particles, fields, energies, history rows, records, traces, gradients, tangents.
KE alone (and history column 0, and a record's KE) is a float64 sum in the launch geometry's order and gets the rtol of
tests/test_gpu_alternate_stores.py.  tests/test_alternate_paths_cpu.py holds the parts these calls are cut into: the tables
are imported from there, so that a case meant to alternate cannot quietly stop doing so.
"""
import os
import re

import numpy as np
import pytest

import hp_adjoint as ha
import hp_mlp_policy as hm
from conftest import record_measure
from test_alternate_paths_cpu import (BOTH_ALTERNATE, BOTH_CASES, FIRST_STEP_CALLS, RECORDER_CALLS, RECORDER_STRIDE,
                                      RECORDER_STRIDE_SINGLE, SINGLE_T, TANGENT_EVERY, TAPE_DRIVES, TAPE_EVERY, TAPE_T, call_sequence,
                                      parts, resolved_every)

pytestmark = pytest.mark.gpu

ALT = dict(readonly_c="on", alternate_stores="on")
STORING = dict(readonly_c="off", alternate_stores="off")
L, NG, E = 50.0, 64, 2
EINVAL = -1

# N, blocks_per_env, dtype, position_dtype: the smallest shapes at which the loops of the non-storing sweeps have all their parts
# (tests/test_gpu_alternate_stores.py: LOOP_CASES)
F64_A = (5003, 2, "float64", None)            # nfull 3 | 1, a partial tile and a lane tail
F64_B = (2049, 1, "float64", None)            # one uniform tile and a one-particle tail
F32 = (10006, 2, "float32", None)
U32 = (12290, 3, "float32", "fixed32")
SHAPES = [F64_A, F64_B, F32, U32]
F64_SHAPES = [F64_A, F64_B]


def _id(shape):
    N, bpe, dtype, pos = shape
    return "%s-N%d-bpe%d" % (pos or dtype, N, bpe)


@pytest.fixture(scope="module")
def oc():
    import ocplasma_amd
    return ocplasma_amd


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


def _same_ke(a, b, dtype):
    assert np.allclose(a, b, rtol=1e-13 if dtype == "float64" else 1e-6, atol=0)


def _same_dicts(ds, what):
    """Bit equality of every entry of the dicts (or lists of arrays) the handles returned."""
    for d in ds[1:]:
        assert len(d) == len(ds[0])
        for k in (ds[0] if isinstance(ds[0], dict) else range(len(ds[0]))):
            assert np.array_equal(np.asarray(ds[0][k]), np.asarray(d[k]), equal_nan=True), (what, k)


def _same_records(recs, dtype):
    from ocplasma_amd.env.record import Record
    for r in recs[1:]:
        for k in Record._ARRAYS:
            a, b = getattr(recs[0], k), getattr(r, k)
            if k == "KE":
                _same_ke(a, b, dtype)
            else:
                assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), k


def _initial(shape, seed):
    """v ~ N(0, 1.5); environment 0 carries the edge vector and the two 40-particle bands next to 0 and L of
    tests/test_gpu_alternate_stores.py::test_alternate_edge_positions, so that the re-derived wrap meets them."""
    N, _, dtype, _ = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, L, (E, N))
    v = rng.normal(0, 1.5, (E, N))
    edge = np.array([0.0, -0.0, np.nextafter(L, 0.0), 1e-300, L - 1e-12, 1e-12, np.nextafter(0.0, 1.0)])
    x[0, :edge.size] = edge
    v[0, :edge.size] = [0.0, 0.0, 0.0, -1.0, 1.0, -1.0, -2.0]
    x[0, 100:140] = np.linspace(L - 0.02, L - 1e-9, 40)        # whole waves within one drift of the edge
    v[0, 100:140] = 0.5
    x[0, 200:240] = np.linspace(1e-9, 0.02, 40)
    v[0, 200:240] = -0.5
    x = x.astype(dtype)
    x[x >= L] = 0.0
    return x, v.astype(dtype)


def _envs(oc, shape, interpol="CIC", M=3, resident=True, **kw):
    """[the handle under test, its storing twin, the resident handle (N <= 8192, where `resident` allows it)]"""
    N, bpe, dtype, pos = shape
    base = dict(L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=interpol, **kw)
    envs = [oc.BatchedPIC(E, N, NG, blocks_per_env=bpe, **ALT, **base), oc.BatchedPIC(E, N, NG, blocks_per_env=bpe, **STORING, **base)]
    assert envs[0]._h.schedule() == "streaming"
    if resident and N <= 8192:
        envs.append(oc.BatchedPIC(E, N, NG, blocks_per_env=-1, **base))
        assert envs[2]._h.schedule() == "resident"
    if M:
        act = oc.E_field(L, NG, M)
        for env in envs:
            env.set_actuator(act)
    return envs


def _close(envs):
    for env in envs:
        assert env.bad_count() == 0
        env.close()


def _fields(rng, T):
    """One random field per step, its amplitude and sign clearly the step's own."""
    amp = 0.02 * (1.0 + np.arange(T)) * (-1.0) ** np.arange(T)
    return amp[:, None, None] * rng.normal(size=(T, E, NG))


def _ext_traj_device(env, traj):
    """pic_step_ext_traj on a trajectory in device memory."""
    import torch
    from ocplasma_amd import _abi
    t = torch.as_tensor(np.ascontiguousarray(traj, dtype=np.float64), device=f"cuda:{env.device}")
    torch.cuda.synchronize()
    h = env._h
    h._chk(h.lib.pic_step_ext_traj(h._h, _abi._ptr(int(t.data_ptr())), _abi.PIC_DEVICE, int(traj.shape[0]), None, None))
    env.sync()                                   # (t must outlive the steps that read it)


# ---- a. per-step fields -------------------------------------------------------------------------------------------------------
FIELD_CASES = [(s, "CIC") for s in SHAPES] + [(s, "TSC") for s in (F64_A, F32, U32)]


@pytest.mark.parametrize("shape,interpol", FIELD_CASES, ids=[_id(s) + "-" + i for s, i in FIELD_CASES])
def test_per_step_fields(oc, shape, interpol):
    """step_ext_traj for T = 2 ... 7 (T = 2 has no Y step): B2_RD of step s re-derives sweep D of step s - 1 under that step's
    field and then pushes under its own."""
    dtype = shape[2]
    envs = _envs(oc, shape, interpol, M=0)
    x0, v0 = _initial(shape, seed=shape[0])
    rng = np.random.default_rng(shape[0] + 1)
    for env in envs:
        env.reset(x0, v0)
    for T in range(2, 8):
        traj = _fields(rng, T)
        _same_hist([env.step_ext_traj(traj, history=True) for env in envs], dtype)
        for other in envs[1:]:
            _same(envs[0], other, dtype)
    traj = _fields(rng, 5)                       # the same from device memory: X Y X Y X
    _ext_traj_device(envs[0], traj)
    for env in envs[1:]:
        env.step_ext_traj(traj)
    for other in envs[1:]:
        _same(envs[0], other, dtype)
    _close(envs)


# ---- b. a recorder cuts the calls -----------------------------------------------------------------------------------------------
RECORDER_CASES = [(s, RECORDER_STRIDE) for s in SHAPES] + [(F64_A, RECORDER_STRIDE_SINGLE)]


@pytest.mark.parametrize("shape,stride", RECORDER_CASES, ids=[_id(s) + "-stride%d" % k for s, k in RECORDER_CASES])
def test_recorder_cuts(oc, shape, stride):
    """step(ext, 5), step_actions_traj(7), step_history(None, 4), step_ext_traj(6) under a recorder of stride 3 (parts 3+2, 1+3+3,
    3+1, 2+3+1: test_alternate_paths_cpu.py) and of stride 1 (single steps: the read-only C alone): every record and the state."""
    dtype = shape[2]
    assert [op for op, _ in RECORDER_CALLS] == ["e", "a", "s", "p"] and [n for _, n in RECORDER_CALLS] == [5, 7, 4, 6]
    assert all((max(ps) >= 3) == (stride == 3) for _, ps in call_sequence(RECORDER_CALLS, stride=stride))
    envs = _envs(oc, shape)
    x0, v0 = _initial(shape, seed=shape[0] + 2)
    rng = np.random.default_rng(shape[0] + 3)
    ext = 0.05 * rng.normal(size=(E, NG))
    a = rng.uniform(-1.0, 1.0, (7, E, 6))
    traj = _fields(rng, 6)
    hs = []
    for env in envs:
        env.reset(x0, v0)
        env.start_recording(stride=stride, modes=4, x_bins=16, v_bins=16, phase_bins=(16, 12), vmin=-6.0, vmax=6.0, capacity=32)
        env.step(ext, 5)
        env.step_actions_traj(a)
        hs.append(env.step_history(None, 4))
        env.step_ext_traj(traj)
    recs = [env.recorded() for env in envs]
    assert np.array_equal(recs[0].steps, np.arange(stride, 23, stride))
    _same_records(recs, dtype)
    _same_hist(hs, dtype)
    for other in envs[1:]:
        _same(envs[0], other, dtype)
    for env in envs:
        env.stop_recording()
    _close(envs)


# ---- c. the tape: forward, replay, adjoint ------------------------------------------------------------------------------------
def _tape_inputs(shape, seed):
    N = shape[0]
    rng = np.random.default_rng(seed)
    return dict(a=rng.uniform(-0.5, 0.5, (TAPE_T, E, 6)), traj=_fields(rng, TAPE_T), ext=0.05 * rng.normal(size=(E, NG)),
                cot=rng.standard_normal((TAPE_T, 3, E)), cx=rng.standard_normal((E, N)), cv=rng.standard_normal((E, N)))


def _drive(env, kind, p):
    if kind == "actions":
        return env.step_actions_traj(p["a"], history=True)
    if kind == "ext_traj":
        return env.step_ext_traj(p["traj"], history=True)
    env.step(p["ext"], TAPE_T)                   # a held field
    return None


def _clean(env, T):
    st = env.tape_stats()
    assert st["steps"] == T and st["replay_mismatches"] == 0 and st["replay_bad_positions"] == 0 and st["unit_retries"] == 0, st


@pytest.mark.parametrize("every", TAPE_EVERY)
@pytest.mark.parametrize("shape", F64_SHAPES, ids=_id)
def test_tape_replay_and_adjoint(oc, shape, every):
    """Seven taped steps in parts of 3+3+1, 1 x 7, 4+3 or 7 (checkpoint_every 0 and 3, 1, 4, 7), driven by per-step actions, by
    per-step fields and by a held field: adjoint_replay_kernel reproduces the forward made of re-derived sub-stages, and the
    gradient has the bits of the storing and of the resident handle.  One case is held to the autograd oracle."""
    import test_gpu_adjoint as tga
    ev = resolved_every(TAPE_T, every)
    assert (max(parts(TAPE_T, every=ev)) >= 3) == (every != 1)
    envs = _envs(oc, shape)
    x0, v0 = _initial(shape, seed=shape[0] + 4)
    p = _tape_inputs(shape, shape[0] + every)
    for kind in TAPE_DRIVES:
        hs, gs = [], []
        for env in envs:
            env.reset(x0, v0)
            env.start_tape(TAPE_T, every)
            assert env.tape_stats()["checkpoint_every"] == ev
            hs.append(_drive(env, kind, p))
            gs.append(env._h.tape_backward(p["cot"], p["cx"], p["cv"], ext=True, actions=True, particles=True))
            _clean(env, TAPE_T)
        if hs[0] is not None:
            _same_hist(hs, "float64")
        for other in envs[1:]:
            _same(envs[0], other, "float64")
        _same_dicts(gs, kind)
        for env in envs:
            env.stop_tape()
        if shape == F64_A and every == 4 and kind == "actions":
            ext = tga._ext_of(p["a"], NG)
            S = ha.Setup(shape[0], NG, L, 1.0, envs[0].dt)
            worst = 0.0
            for e in range(E):
                ge, gx, gv = ha.autograd_vjp(x0[e], v0[e], ext[:, e], S, p["cot"][:, :, e], p["cx"][e], p["cv"][e])
                worst = max(worst, tga._rel(gs[0]["g_ext"][:, e], ge), tga._rel(gs[0]["g_actions"][:, e], tga._bt(ge, NG)),
                            tga._rel(gs[0]["g_x0"][e], gx), tga._rel(gs[0]["g_v0"][e], gv))
            record_measure("alternate.adjoint_parity", worst)
            print(f"alternate.adjoint_parity = {worst:.3e} (bound {tga.PARITY_BOUND:.1e})")
            assert worst < tga.PARITY_BOUND, worst
    _close(envs)


# ---- d. the tape: forward mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", TANGENT_EVERY)
@pytest.mark.parametrize("shape", F64_SHAPES, ids=_id)
def test_tape_forward_mode(oc, shape, every):
    """`tangent` over the whole tape and a `tangent_walk` stepped to its end, on parts of 3+3+1 and of 7."""
    assert max(parts(TAPE_T, every=resolved_every(TAPE_T, every))) >= 3
    N = shape[0]
    envs = _envs(oc, shape)
    x0, v0 = _initial(shape, seed=N + 5)
    p = _tape_inputs(shape, N + 10 + every)
    rng = np.random.default_rng(N + 6)
    da, dx, dv = rng.standard_normal((TAPE_T, E, 6)), rng.standard_normal((E, N)), rng.standard_normal((E, N))
    whole, steps, ends = [], [], []
    for env in envs:
        env.reset(x0, v0)
        env.start_tape(TAPE_T, every)
        env.step_actions_traj(p["a"])
        whole.append(env.tangent(d_actions=da, d_x0=dx, d_v0=dv, fields=True))
        _clean(env, TAPE_T)
        walk = env.tangent_walk(d_x0=dx, d_v0=dv)
        out = {}
        for t in range(TAPE_T):
            r = walk.step(d_actions=da[t], state=True, fields=True)
            assert r["t"] == t
            out.update({"%s[%d]" % (k, t): a for k, a in r.items()})
        steps.append(out)
        ends.append(list(walk.end()))
        _clean(env, TAPE_T)
    _same_dicts(whole, "tangent")
    _same_dicts(steps, "tangent_walk.step")
    _same_dicts(ends, "tangent_walk.end")
    for other in envs[1:]:
        _same(envs[0], other, "float64")
    for env in envs:
        env.stop_tape()
    _close(envs)


# ---- e. single-step parts under the read-only sweep C -----------------------------------------------------------------------------
def _pair(oc, shape, M=2):
    return _envs(oc, shape, M=M, resident=False)


def _cots(N, seed):
    rng = np.random.default_rng(seed)
    T = SINGLE_T
    return dict(d_KE=rng.normal(size=(T, E)), d_PE=rng.normal(size=(T, E)), d_PE_reward=rng.normal(size=(T, E)),
                d_x=rng.normal(size=(E, N)), d_v=rng.normal(size=(E, N)))


def _rows(r):
    return {k: np.asarray(getattr(r, k)) for k in r._fields if k != "KE"}


def test_single_steps_with_a_kl_trace(oc):
    """A tape with a KL attached cuts every step: five parts of one step each, bit for bit the storing twin's -- trace,
    history rows, gradient and state."""
    assert parts(SINGLE_T, every=resolved_every(SINGLE_T, 0), per_step=True) == [1] * SINGLE_T
    N = F64_A[0]
    envs = _pair(oc, F64_A)
    x0, v0 = _initial(F64_A, seed=31)
    rng = np.random.default_rng(32)
    a = rng.uniform(-0.5, 0.5, (SINGLE_T, E, 4))
    c = _cots(N, 33)
    d_kl = rng.normal(size=(SINGLE_T, E))
    envs[1].reset(x0, v0)
    feq = envs[1].phase_density_smooth((16, 12), -6.0, 6.0)[0]
    hs, kls, gs = [], [], []
    for env in envs:
        env.reset(x0, v0)
        env.start_tape(SINGLE_T, 0, kl=dict(feq=feq, vmin=-6.0, vmax=6.0))
        hs.append(env.step_actions_traj(a, history=True))
        kls.append(env.tape_kl())
        gs.append(env.backward(d_KL=d_kl, **c))
        _clean(env, SINGLE_T)
    _same_hist(hs, "float64")
    assert np.array_equal(kls[0], kls[1]) and np.all(np.isfinite(kls[0]))
    _same_dicts(gs, "backward")
    _same(envs[0], envs[1], "float64")
    for env in envs:
        env.stop_tape()
    _close(envs)


def test_single_steps_with_a_moments_trace(oc):
    assert parts(SINGLE_T, every=resolved_every(SINGLE_T, 0), per_step=True) == [1] * SINGLE_T
    N = F64_A[0]
    envs = _pair(oc, F64_A)
    x0, v0 = _initial(F64_A, seed=41)
    rng = np.random.default_rng(42)
    traj = _fields(rng, SINGLE_T)
    c = _cots(N, 43)
    d_m = rng.normal(size=(SINGLE_T, E, 3, NG))
    hs, ms, gs = [], [], []
    for env in envs:
        env.reset(x0, v0)
        env.start_tape(SINGLE_T, 0, moments=True)
        hs.append(env.step_ext_traj(traj, history=True))
        ms.append(env.tape_moments())
        gs.append(env.backward(d_moments=d_m, **c))
        _clean(env, SINGLE_T)
    _same_hist(hs, "float64")
    assert np.array_equal(ms[0], ms[1]) and np.all(np.isfinite(ms[0]))
    _same_dicts(gs, "backward")
    _same(envs[0], envs[1], "float64")
    for env in envs:
        env.stop_tape()
    _close(envs)


def test_single_steps_of_a_taped_policy(oc):
    """tape_step_policy steps one step at a time; backward_policy and tape_policy_grad behind it."""
    from ocplasma_amd.control.policy import MLPPolicy
    N = F64_B[0]
    widths = [4, 8, 4]
    pol = MLPPolicy(widths, "tanh", hm.make_params(widths, 5), 2, squash=True, action_scale=1.25)
    envs = _pair(oc, F64_B)
    x0, v0 = _initial(F64_B, seed=51)
    rng = np.random.default_rng(52)
    eps, std = rng.normal(size=(SINGLE_T, E, 4)), rng.uniform(0.05, 0.3, 4)
    c = _cots(N, 53)
    d_a = 0.1 * rng.normal(size=(SINGLE_T, E, 4))
    rs, gs, gps = [], [], []
    for env in envs:
        env.reset(x0, v0)
        env.start_tape(SINGLE_T, 0)
        rs.append(env.tape_step_policy(pol, SINGLE_T, noise=eps, std=std))
        gs.append(env.backward_policy(d_actions=d_a, **c))
        gps.append(env.tape_policy_grad())
        _clean(env, SINGLE_T)
    _same_dicts([_rows(r) for r in rs], "tape_step_policy")
    _same_ke(rs[0].KE, rs[1].KE, "float64")
    _same_dicts(gs, "backward_policy")
    assert np.array_equal(gps[0], gps[1]) and np.array_equal(gps[0], gs[0]["params"]) and np.any(gps[0] != 0.0)
    _same(envs[0], envs[1], "float64")
    for env in envs:
        env.stop_tape()
    _close(envs)


def test_single_steps_of_the_particle_actor(oc):
    """step_actor with the rollout actor of tests/test_gpu_actor.py: features, pre-activations, actions and energies of every
    step, and the state."""
    import test_gpu_actor as tga
    actor = tga._rollout_actor()
    envs = _pair(oc, F64_A, M=tga.M3)
    x0, v0 = _initial(F64_A, seed=61)
    rng = np.random.default_rng(62)
    eps, std = rng.normal(size=(SINGLE_T, E, 2 * tga.M3)), rng.uniform(0.05, 0.3, 2 * tga.M3)
    rs = []
    for env in envs:
        env.reset(x0, v0)
        rs.append(env.step_actor(actor, SINGLE_T, noise=eps, std=std))
    _same_dicts([_rows(r) for r in rs], "step_actor")
    _same_ke(rs[0].KE, rs[1].KE, "float64")
    assert np.all(np.isfinite(rs[0].actions)) and np.ptp(rs[0].actions) > 0
    _same(envs[0], envs[1], "float64")
    _close(envs)


# ---- f. a tape and a recorder together ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,every", BOTH_CASES)
def test_tape_and_recorder_together(oc, stride, every):
    """One step_actions_traj of seven steps cut by both.  Stride 2 and checkpoint_every 3 cut it into 2+1+1+2+1 (no Y step: the
    read-only C alone); stride 3 and checkpoint_every 4 into 3+1+2+1."""
    ps = parts(7, 0, stride, 0, resolved_every(7, every))
    assert (max(ps) >= 3) == BOTH_ALTERNATE[stride, every], ps
    envs = _envs(oc, F64_A)
    x0, v0 = _initial(F64_A, seed=71)
    p = _tape_inputs(F64_A, 72 + stride)
    hs, gs = [], []
    for env in envs:
        env.reset(x0, v0)
        env.start_recording(stride=stride, modes=4, x_bins=16, v_bins=16, phase_bins=(16, 12), vmin=-6.0, vmax=6.0, capacity=8)
        env.start_tape(7, every)
        hs.append(env.step_actions_traj(p["a"], history=True))
        gs.append(env._h.tape_backward(p["cot"], p["cx"], p["cv"], ext=True, actions=True, particles=True))
        _clean(env, 7)
    recs = [env.recorded() for env in envs]
    assert np.array_equal(recs[0].steps, np.arange(stride, 8, stride))
    _same_records(recs, "float64")
    _same_hist(hs, "float64")
    _same_dicts(gs, "tape_backward")
    for other in envs[1:]:
        _same(envs[0], other, "float64")
    for env in envs:
        env.stop_tape()
        env.stop_recording()
    _close(envs)


# ---- g. a first step without a cached deposit -----------------------------------------------------------------------------------
def _drop_invalidate(env, src, rng):
    env.invalidate()


def _drop_set_particles(env, src, rng):
    x, v = _initial((env.N, 0, env.dtype, None), seed=int(rng.integers(1 << 30)))
    env._h.set_particles(x, v)                   # (no refresh: the fields stay the old particles')


def _drop_copy_from(env, src, rng):
    src.step(None, 2)
    src.invalidate()                             # the source holds no cached deposit: the copy drops the destination's
    env.copy_from(src, np.array([1, 0]))


def _drop_fork(env, src, rng):
    """It is invalidate() that drops the deposit (a fork of a handle with one keeps it); the fork behind it copies environment 1
    over environment 0 and must leave the handle without one."""
    env.invalidate()
    env.fork(np.array([1, 1]))


DROPS = {"invalidate": _drop_invalidate, "set_particles": _drop_set_particles, "copy_from": _drop_copy_from, "fork": _drop_fork}


@pytest.mark.parametrize("drop", sorted(DROPS))
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_first_step_deposits_q1_itself(oc, shape, drop):
    """After an alternating call of 4 the cached q1 deposit goes; step(ext, 5) and step_actions_traj(6) then open with the sweep
    ST_A in front of their X Y pattern."""
    assert FIRST_STEP_CALLS == [("s", 4), ("e", 5), ("s", 4), ("a", 6)]
    N, bpe, dtype, pos = shape
    envs = _envs(oc, shape)
    x0, v0 = _initial(shape, seed=N + 7)
    rng = np.random.default_rng(N + 8)
    ext = 0.05 * rng.normal(size=(E, NG))
    a = rng.uniform(-1.0, 1.0, (6, E, 6))
    envs[0].profile(True)
    for env in envs:
        src = oc.BatchedPIC(E, N, NG, L=L, dt=0.1, dtype=dtype, position_dtype=pos, blocks_per_env=1, **STORING)
        src.reset(*_initial(shape, seed=N + 9))
        seeds = np.random.default_rng(N + 10)    # (every handle gets the same new particles)
        env.reset(x0, v0)
        env.step(None, 4)
        DROPS[drop](env, src, seeds)
        env.step(ext, 5)
        env.sync()
        src.close()
    for other in envs[1:]:
        _same(envs[0], other, dtype)
    for env in envs:
        src = oc.BatchedPIC(E, N, NG, L=L, dt=0.1, dtype=dtype, position_dtype=pos, blocks_per_env=1, **STORING)
        src.reset(*_initial(shape, seed=N + 11))
        seeds = np.random.default_rng(N + 12)
        env.step(None, 4)
        DROPS[drop](env, src, seeds)
        env.step_actions_traj(a)
        env.sync()
        src.close()
    for other in envs[1:]:
        _same(envs[0], other, dtype)
    # the two calls under test, and no other, opened with a sweep A (test_alternate_paths_cpu.py counts the same in the plan)
    assert envs[0].profile_read()["sweep_A"][1] == 2
    _close(envs)


# ---- h. where the mode must not engage --------------------------------------------------------------------------------------------
def test_verlet_ignores_the_mode(oc):
    envs = _envs(oc, F64_A, resident=False, integrator="verlet")
    x0, v0 = _initial(F64_A, seed=81)
    rng = np.random.default_rng(82)
    ext = 0.05 * rng.normal(size=(E, NG))
    a = rng.uniform(-1.0, 1.0, (6, E, 6))
    hs = []
    for env in envs:
        env.reset(x0, v0)
        env.step(ext, 5)
        hs.append(env.step_actions_traj(a, history=True))
    _same_hist(hs, "float64")
    _same(envs[0], envs[1], "float64")
    _close(envs)


def test_gain_law_tape_ignores_the_mode(oc):
    """The feedback law needs each step's field: a step_feedback_gain call falls back to the storing schedule, under a tape too."""
    N = F64_A[0]
    envs = _envs(oc, F64_A, M=2, resident=False)
    x0, v0 = _initial(F64_A, seed=83)
    rng = np.random.default_rng(84)
    G = np.diag([-1.0, -1.0, 1.0, 1.0])[None] + 0.1 * rng.normal(size=(E, 4, 4))
    c = _cots(N, 85)
    T = SINGLE_T
    d_modes = rng.normal(size=(T, E, 4))
    fs, gs = [], []
    for env in envs:
        env.reset(x0, v0)
        env.start_tape(T, 3)
        fs.append(env.step_feedback_gain(G, T, actions=True, modes=True, history=True))
        gs.append(env.backward(d_modes=d_modes, **c))
        _clean(env, T)
    _same_ke(fs[0].pop("KE"), fs[1].pop("KE"), "float64")
    _same_dicts(fs, "step_feedback_gain")
    _same_dicts(gs, "backward")
    _same(envs[0], envs[1], "float64")
    for env in envs:
        env.stop_tape()
    _close(envs)


def _first_ng_without_room():
    """The smallest float64 mesh whose sweeps fit the LDS but not with the second field tile, from host_plan.h's formula:
    sweep_lds = 2 R (Ng + 2) 8 + (Ng + 2) esz with R = 1 and esz = 8; the re-deriving sweeps need (Ng + 2) esz more; either plus
    kSweepStaticLds = (2 WAVES + 2) 8 must not exceed kLdsLimit (pic_limits.h)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "optimal-control-1d-electrostatic-plasma_amd", "csrc", "pic_limits.h")).read()
    m_block = re.search(r"constexpr int BLOCK = (\d+);", text)
    m_limit = re.search(r"constexpr size_t kLdsLimit = ([\d* ]+);", text)
    assert m_block and m_limit, "pic_limits.h no longer spells BLOCK or kLdsLimit as this test reads them: update the patterns"
    assert re.search(r"kSweepStaticLds = \(2 \* WAVES \+ 2\) \* sizeof\(double\)", text) and "WAVES = BLOCK / 64" in text, \
        "pic_limits.h no longer spells kSweepStaticLds or WAVES as this test restates them"
    plan = open(os.path.join(root, "optimal-control-1d-electrostatic-plasma_amd", "csrc", "host_plan.h")).read()
    assert "p->sweep_lds = 2 * p->R * stride * 8 + stride * p->esz;" in plan and \
        "p->sweep_lds + stride * p->esz + kSweepStaticLds <= kLdsLimit" in plan, \
        "host_plan.h no longer sizes the sweeps' LDS as this test restates it (24 and 32 bytes per cell in float64)"
    block = int(m_block.group(1))
    limit = int(np.prod([int(f) for f in m_limit.group(1).split("*")]))
    static = (2 * (block // 64) + 2) * 8
    fits = lambda ng: 24 * (ng + 2) + static <= limit
    fits_rc = lambda ng: 32 * (ng + 2) + static <= limit
    ng = next(n for n in range(2, limit) if not fits_rc(n))
    assert fits(ng) and fits_rc(ng - 1)
    return ng


def test_mesh_without_room_for_the_second_tile(oc):
    """pic_set_readonly_c(ON) and pic_set_alternate_stores(ON) are refused with PIC_EINVAL where the second field tile does not
    fit, and the handle then steps as one that was never asked; one cell fewer and both are accepted."""
    from ocplasma_amd._abi import PicError
    ng = _first_ng_without_room()
    N = F64_B[0]
    kw = dict(L=L, dt=0.1, blocks_per_env=1)
    asked, never, fits = oc.BatchedPIC(1, N, ng, **kw), oc.BatchedPIC(1, N, ng, **kw), oc.BatchedPIC(1, N, ng - 1, **kw)
    fits._h.set_readonly_c("on")
    fits._h.set_alternate_stores("on")
    fits.close()
    with pytest.raises(PicError, match=r"libpicstep error %d: pic_set_alternate_stores: Ng too large for the second field tile of "
                                       r"sweeps C_RB and B2_RD" % EINVAL):
        asked._h.set_alternate_stores("on")
    with pytest.raises(PicError, match=r"libpicstep error %d: pic_set_readonly_c: Ng too large for the second field tile of sweep "
                                       r"D_RC" % EINVAL):
        asked._h.set_readonly_c("on")
    rng = np.random.default_rng(91)
    x0 = rng.uniform(0, L, (1, N))
    v0 = rng.normal(0, 1.5, (1, N))
    ext = 0.05 * rng.normal(size=(1, ng))
    hs = []
    for env in (asked, never):
        env.reset(x0, v0)
        env.step(ext, 5)
        hs.append(env.step_history(None, 4))
    assert all(np.array_equal(a, b) for a, b in zip(*hs))
    (xa, va), (xb, vb) = asked.particles(), never.particles()
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    _same(asked, never, "float64")
    for env in (asked, never):
        assert env.bad_count() == 0
        env.close()
