"""The device's derivatives at the edge shapes and off-default parameters of tests/hp_grad_cases.py (last
paragraph): the adjoint, the forward mode, the per-step smoothed KL and the fluid moments in both modes, the actuator and the
gain law, each against the float64 restatement its own GPU test uses, and bitwise invariants that need no reference.  The premises
(the references' own floor, no reference position within a rounding of a node) are pinned by tests/test_grad_edges_cpu.py.

Bound of a comparison: max(the bound the surface's own GPU test asserts, 100 x the case's floor), never above 1e-9; the floor is
the references' hand equations against automatic differentiation at that case (hp_grad_cases.floors), a quantity of the
references alone.  The faults this matrix is after (a dropped n0, a wrong fold at node Ng, a row offset by ld - N, an environment
reading its neighbour's unit) give errors of 1e-2 to 1.  Every measured error and floor is recorded under
grad_edges.<case>.<surface> and listed in profiles/grad_edges.md.

A tape is driven by step_ext_traj: no actuator exists on a mesh of 4 or 5 nodes.  Device results are computed once per
(case, schedule, checkpoint interval, environments) and shared by the tests; nothing modifies them."""
import functools

import numpy as np
import pytest
import torch

import hp_feedback as hf
import hp_grad_cases as gc
import hp_moments as hm
import hp_moments_jvp as hj
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

# the bounds the surfaces' own GPU tests assert, restated (each is 100 x what that test measured)
ADJOINT_BOUND = 1.3e-11       # test_gpu_adjoint.py: PARITY_BOUND
TANGENT_BOUND = 6.2e-11       # test_gpu_tangent.py: PARITY_BOUND
KL_TRACE_BOUND = 3.4e-14      # test_gpu_tape_kl.py: TOL_KL (max-abs over the trace, as there)
KL_GRAD_BOUND = 4.5e-12       # test_gpu_tape_kl.py: GRAD_BOUND
KL_TANGENT_BOUND = 5.3e-12    # test_gpu_tangent_kl.py: PARITY_BOUND
MOMENTS_GRAD_BOUND = 9.0e-13  # test_gpu_moments.py: TAPE_BOUND
MOMENTS_TANGENT_BOUND = 1.5e-11   # test_gpu_moments_jvp.py: TAPE_BOUND
GAIN_BOUND = 3e-12            # test_gpu_feedback_gain.py: PARITY_BOUND
GAIN_FORWARD_BOUND = 1e-9     # test_gpu_feedback_gain.py: the forward's modes and actions against the restatement

PLAIN = [(cid, s) for cid, c in gc.CASES.items() for s in c.schedules]
M = 2                         # actuator modes of case C's closed-loop tests


def _ids(pairs):
    return [f"{cid}-bpe{s}" for cid, s in pairs]


def _make(cid, sched, envs=None, actuator=False):
    """A handle of case cid's environments `envs` (all by default) with the case's L, n0 and dt, not clamped."""
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    c, i = gc.CASES[cid], gc.inputs(cid)
    sel = slice(None) if envs is None else list(envs)
    X, V = np.ascontiguousarray(i["x"][sel]), np.ascontiguousarray(i["v"][sel])
    env = BatchedPIC(X.shape[0], c.N, c.Ng, n0=c.n0, L=c.L, dt=c.dt, blocks_per_env=sched)
    assert env.dt == c.dt and env.n0 == c.n0 and env.L == c.L, (env.dt, c.dt)
    if sched > 0:
        assert env._h.schedule() == "streaming"
    env.reset(X, V)
    if actuator:
        env.set_actuator(oc.E_field(c.L, c.Ng, M))
    return env


def _healthy(env):
    st = env.tape_stats()
    assert st["replay_mismatches"] == 0 and st["unit_retries"] == 0 and st["replay_bad_positions"] == 0, st
    return st


def _sel(i, envs):
    """The batch inputs restricted to `envs`, every array contiguous."""
    if envs is None:
        return i
    e = list(envs)
    ax = {"ext": 1, "d_ext": 1, "ckl": 1, "cmom": 1, "cot": 2}
    return {k: (a if k == "feq" else np.ascontiguousarray(np.take(a, e, axis=ax.get(k, 0)))) for k, a in i.items()}


def _energy_cots(i):
    return dict(d_KE=i["cot"][:, 0], d_PE=i["cot"][:, 1], d_PE_reward=i["cot"][:, 2], d_x=i["cx"], d_v=i["cv"])


def _directions(i):
    z = np.zeros_like
    return dict(d_ext=np.stack([i["d_ext"], z(i["d_ext"]), i["d_ext"]]), d_x0=np.stack([z(i["d_x0"]), i["d_x0"], z(i["d_x0"])]),
                d_v0=np.stack([z(i["d_v0"]), z(i["d_v0"]), i["d_v0"]]))


@functools.lru_cache(maxsize=None)
def _plain(cid, sched, every=None, envs=None):
    """(backward, tangent) of a plain tape of the case: cotangents on the three energy traces and the final x, v; K = 3 directions
    (d_ext alone, d_x0 alone, d_v0 with d_ext) in one call, with every step's field tangent."""
    c = gc.CASES[cid]
    i = _sel(gc.inputs(cid), envs)
    env = _make(cid, sched, envs)
    env.start_tape(c.T, c.every if every is None else every)
    env.step_ext_traj(i["ext"])
    g = env.backward(**_energy_cots(i))
    _healthy(env)
    t = env.tangent(fields=True, **_directions(i))
    st = _healthy(env)
    assert st["steps"] == c.T, st
    env.stop_tape()
    env.close()
    return g, t


def _hist(t, k, e):
    return np.stack([t["KE"][k][:, e], t["PE"][k][:, e], t["PE_reward"][k][:, e]], axis=1)       # [T, 3]


def _check(cid, sched, surface, err, surface_bound, floor_name):
    """Record the device's error and the floor, then assert the bound of the module's docstring."""
    b = gc.bound(cid, surface_bound, floor_name)
    fl = gc.floors(cid)[floor_name]
    name = f"grad_edges.{cid}.{surface}.bpe{sched}"
    print(f"{name}: device {err:.3e}  floor {fl:.3e}  bound {b:.3e}")
    record_measure(name, err)
    record_measure(f"grad_edges.{cid}.floor.{floor_name}", fl)
    record_measure(name + ".bound", b)
    assert err < b, (name, err, b)


# ---- 1. parity with the references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,sched", PLAIN, ids=_ids(PLAIN))
def test_backward_matches_autograd(cid, sched):
    c = gc.CASES[cid]
    g, _ = _plain(cid, sched)
    worst = 0.0
    for e in c.ref_envs:
        ge, gx, gv = gc.ref_adjoint(cid, e)
        worst = max(worst, gc.rel(g["ext"][:, e], ge), gc.rel(g["x0"][e], gx), gc.rel(g["v0"][e], gv))
    _check(cid, sched, "backward", worst, ADJOINT_BOUND, "adjoint")


@pytest.mark.parametrize("cid,sched", PLAIN, ids=_ids(PLAIN))
def test_tangent_matches_forward_mode(cid, sched):
    c = gc.CASES[cid]
    _, t = _plain(cid, sched)
    worst = 0.0
    for e in c.ref_envs:
        for k, (h, x, v, m) in enumerate(gc.ref_tangent(cid, e)):
            worst = max(worst, gc.rel(_hist(t, k, e), h), gc.rel(t["x"][k][e], x), gc.rel(t["v"][k][e], v),
                        gc.rel(t["E_mesh"][k][:, e], m))
    _check(cid, sched, "tangent", worst, TANGENT_BOUND, "tangent")


KLS = [(cid, s) for cid in gc.KL_CASES for s in gc.CASES[cid].schedules]


@pytest.mark.parametrize("cid,sched", KLS, ids=_ids(KLS))
def test_kl_trace_gradient_and_tangent_match_the_restatement(cid, sched):
    """A tape with the smoothed KL on a 16 x 16 grid over +-0.12 L, hp_phase.Grid given the case's n0: the trace, backward with a
    cotangent on it (and on the energies and the final particles) and tangent(kl=True)."""
    c, i = gc.CASES[cid], gc.inputs(cid)
    lo, hi = c.vrange
    env = _make(cid, sched)
    env.start_tape(c.T, c.every, kl=dict(feq=i["feq"], vmin=lo, vmax=hi))
    env.step_ext_traj(i["ext"])
    trace = env.tape_kl()
    g = env.backward(d_KL=i["ckl"], **_energy_cots(i))
    _healthy(env)
    t = env.tangent(kl=True, **_directions(i))
    _healthy(env)
    env.stop_tape()
    env.close()
    assert trace.shape == (c.T, c.E) and t["KL"].shape == (3, c.T, c.E)
    e_tr = e_g = e_t = 0.0
    for e in c.ref_envs:
        want, (ge, gx, gv) = gc.ref_tape_kl(cid, e)
        e_tr = max(e_tr, float(np.max(np.abs(trace[:, e] - want)) / np.max(np.abs(want))))
        e_g = max(e_g, gc.rel(g["ext"][:, e], ge), gc.rel(g["x0"][e], gx), gc.rel(g["v0"][e], gv))
        for k, dkl in enumerate(gc.ref_tangent_kl(cid, e)):
            assert np.any(dkl != 0.0)
            e_t = max(e_t, gc.rel(t["KL"][k][:, e], dkl))
    _check(cid, sched, "kl_trace", e_tr, KL_TRACE_BOUND, "tape_kl")
    _check(cid, sched, "kl_backward", e_g, KL_GRAD_BOUND, "tape_kl")
    _check(cid, sched, "kl_tangent", e_t, KL_TANGENT_BOUND, "tangent")


MOMS = [(cid, s) for cid in gc.MOMENTS_CASES for s in gc.CASES[cid].schedules]


@pytest.mark.parametrize("cid,sched", MOMS, ids=_ids(MOMS))
def test_moments_gradient_and_tangent_match_the_restatement(cid, sched):
    """A tape with the moments' trace: backward with cotangents on every step's moments and on PE_reward (the cotangents of
    test_gpu_moments.py's tape test), and tangent(moments=True)."""
    c, i = gc.CASES[cid], gc.inputs(cid)
    S = c.setup()
    env = _make(cid, sched)
    env.start_tape(c.T, c.every, moments=True)
    env.step_ext_traj(i["ext"])
    g = env.backward(d_PE_reward=i["cot"][:, 2], d_moments=i["cmom"])
    _healthy(env)
    t = env.tangent(moments=True, **_directions(i))
    _healthy(env)
    env.stop_tape()
    env.close()
    assert t["moments"].shape == (3, c.T, c.E, 3, c.Ng)
    e_g = e_t = 0.0
    for e in c.ref_envs:
        x0, v0, et = (torch.as_tensor(a).clone().requires_grad_(True) for a in (i["x"][e], i["v"][e], i["ext"][:, e]))
        _, _, hist, mom, _ = hm.rollout_moments(x0, v0, et, S)
        J = (mom * torch.as_tensor(i["cmom"][:, e])).sum() + (hist[:, 2] * torch.as_tensor(i["cot"][:, 2, e])).sum()
        ge, gx, gv = (a.numpy() for a in torch.autograd.grad(J, (et, x0, v0)))
        e_g = max(e_g, gc.rel(g["ext"][:, e], ge), gc.rel(g["x0"][e], gx), gc.rel(g["v0"][e], gv))
        for k, u in enumerate(gc.directions(cid, e)):
            want = hj.rollout_torch_jvp(i["x"][e], i["v"][e], i["ext"][:, e], S, **u)
            e_t = max([e_t] + [gc.rel(t["moments"][k, s, e, m], want[s, m]) for s in range(c.T) for m in range(3)])
    _check(cid, sched, "moments_backward", e_g, MOMENTS_GRAD_BOUND, "adjoint")
    _check(cid, sched, "moments_tangent", e_t, MOMENTS_TANGENT_BOUND, "tangent")


def _basis(c):
    bc, bs = po.actuator_basis(c.L, c.Ng, M)
    return np.concatenate([bc, bs], axis=1)                         # B [Ng, 2M]


@pytest.mark.parametrize("sched", gc.CASES["C"].schedules)
def test_case_c_gradient_through_the_actuator(sched):
    """step_actions_traj with two actuator modes on the mesh of 33 nodes in the box of 7.7: g_actions = B^T g_ext of the
    reference under the fields B a_t, and g_x0, g_v0."""
    import hp_adjoint as ha
    cid = "C"
    c, i = gc.CASES[cid], gc.inputs(cid)
    acts = np.random.default_rng([c.N, c.Ng, c.salt, 2 << 20]).uniform(-0.5, 0.5, (c.T, c.E, 2 * M))
    env = _make(cid, sched, actuator=True)
    env.start_tape(c.T, c.every)
    env.step_actions_traj(acts)
    g = env.backward(**_energy_cots(i))
    _healthy(env)
    env.stop_tape()
    env.close()
    B, S = _basis(c), c.setup()
    worst = 0.0
    for e in c.ref_envs:
        ext = np.stack([po.actuator_field(c.L, c.Ng, M, a[:M], a[M:]).ravel() for a in acts[:, e]])
        ge, gx, gv = ha.autograd_vjp(i["x"][e], i["v"][e], ext, S, i["cot"][:, :, e], i["cx"][e], i["cv"][e])
        worst = max(worst, gc.rel(g["actions"][:, e], ge @ B), gc.rel(g["ext"][:, e], ge), gc.rel(g["x0"][e], gx),
                    gc.rel(g["v0"][e], gv))
    _check(cid, sched, "actions", worst, ADJOINT_BOUND, "adjoint")


@pytest.mark.parametrize("sched", gc.CASES["C"].schedules)
def test_case_c_gradient_through_the_gain_law(sched):
    """step_feedback_gain with a random 4 x 4 gain per environment: the gain's gradient, g_x0, g_v0 and the taped modes."""
    cid = "C"
    c, i = gc.CASES[cid], gc.inputs(cid)
    n = 2 * M
    rng = np.random.default_rng([c.N, c.Ng, c.salt, 3 << 20])
    G = np.stack([hf.g0(M) + 0.3 * rng.standard_normal((n, n)) for _ in range(c.E)])
    cm = rng.standard_normal((c.T, c.E, n))
    env = _make(cid, sched, actuator=True)
    env.start_tape(c.T, c.every)
    fwd = env.step_feedback_gain(G, c.T, actions=True, modes=True)
    g = env.backward(d_modes=cm, **_energy_cots(i))
    _healthy(env)
    env.stop_tape()
    env.close()
    assert np.array_equal(g["modes"], fwd["modes"])
    S = c.setup()
    worst = fwd_worst = 0.0
    for e in c.ref_envs:
        wG, wx, wv, wm, wa = hf.autograd_vjp(i["x"][e], i["v"][e], G[e], S, c.T, M, i["cot"][:, :, e], cm[:, e], i["cx"][e], i["cv"][e])
        fwd_worst = max(fwd_worst, gc.rel(fwd["modes"][:, e], wm), gc.rel(fwd["actions"][:, e], wa))
        worst = max(worst, gc.rel(g["gain"][e], wG), gc.rel(g["x0"][e], wx), gc.rel(g["v0"][e], wv))
    _check(cid, sched, "gain_forward", fwd_worst, GAIN_FORWARD_BOUND, "adjoint")
    _check(cid, sched, "gain", worst, GAIN_BOUND, "adjoint")


# ---- 2. exact invariants: no reference, np.array_equal throughout --------------------------------------------------------------
def _same_env(batch, k, alone):
    """Environment k of a batch's (backward, tangent) against the one-environment results `alone`."""
    (gb, tb), (ga, ta) = batch, alone
    for key in ("x0", "v0"):
        assert np.array_equal(gb[key][k], ga[key][0]), key
    assert np.array_equal(gb["ext"][:, k], ga["ext"][:, 0])
    for key in ("KE", "PE", "PE_reward", "E_mesh"):
        assert np.array_equal(tb[key][:, :, k], ta[key][:, :, 0]), key
    for key in ("x", "v"):
        assert np.array_equal(tb[key][:, k], ta[key][:, 0]), key


ALONE = [(cid, s) for cid in "AB" for s in gc.CASES[cid].schedules]


@pytest.mark.parametrize("cid,sched", ALONE, ids=_ids(ALONE))
def test_an_environment_of_a_batch_is_that_environment_alone(cid, sched):
    batch = _plain(cid, sched)
    for k in range(gc.CASES[cid].E):
        _same_env(batch, k, _plain(cid, sched, None, (k,)))


def test_case_g_is_independent_of_the_workgroups_per_environment():
    _same_env(_plain("G", 3), 0, _plain("G", 7))


@pytest.mark.parametrize("cid", ["B", "C"])
def test_checkpoint_interval_does_not_change_a_bit(cid):
    ref = _plain(cid, 0, 1)
    for every in (2, 0):
        got = _plain(cid, 0, every)
        for a, b in zip(ref, got):
            for key in a:
                assert np.array_equal(a[key], b[key]), (every, key)


def test_cotangents_scaled_by_powers_of_two_scale_the_gradients_exactly():
    """Case B: environment 0's cotangents times 2^300, environment 1's times 2^-300, environment 2's times 0.  Every float64
    operation of the reverse pass commutes with a power of two while nothing overflows or underflows, and an environment's
    fixed-point unit is a power of two taken from its own max |c|: the gradients are the unscaled run's bits times 2^300 and
    2^-300, and zeros.  A unit shared between environments, or a zero max taken through the wrong branch, shows here."""
    cid = "B"
    c, i = gc.CASES[cid], gc.inputs(cid)
    s = np.array([2.0 ** 300, 2.0 ** -300, 0.0])
    cots = _energy_cots(i)
    scaled = {k: a * (s[:, None] if k in ("d_x", "d_v") else s[None, :]) for k, a in cots.items()}
    for sched in c.schedules:
        env = _make(cid, sched)
        env.start_tape(c.T, c.every)
        env.step_ext_traj(i["ext"])
        base = env.backward(**cots)
        _healthy(env)
        got = env.backward(**scaled)
        _healthy(env)
        env.stop_tape()
        env.close()
        for key in ("x0", "v0"):
            assert np.array_equal(got[key], base[key] * s[:, None]), (sched, key)
            assert np.all(base[key] != 0.0) and not np.any(got[key][2]) and np.all(np.isfinite(got[key]))
        assert np.array_equal(got["ext"], base["ext"] * s[None, :, None]), sched
        assert not np.any(got["ext"][:, 2]) and np.any(base["ext"][:, 2] != 0.0)
        for key in base:                                              # and the unscaled run is the shared one's bits
            assert np.array_equal(base[key], _plain(cid, sched)[0][key]), (sched, key)


def test_case_h_twin_environments_give_the_same_bits():
    """Environments 0 and 299 hold the same particles, fields, cotangents and tangents, 299 rows apart."""
    g, t = _plain("H", 0)
    last = gc.CASES["H"].E - 1
    one = ({k: np.take(a, [last], axis=1 if k == "ext" else 0) for k, a in g.items()},
           {k: np.take(a, [last], axis=2 if k in ("KE", "PE", "PE_reward", "E_mesh") else 1) for k, a in t.items()})
    _same_env((g, t), 0, one)
    assert not np.array_equal(g["x0"][0], g["x0"][1])
