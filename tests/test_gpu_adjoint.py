"""Differentiable rollouts on the device (pic_tape_*): the adjoint against the autograd oracle
(tests/hp_adjoint.py), against finite differences of the device's own forward, bitwise reproducibility, no perturbation of the
forward, the C contract and the torch Function."""
import numpy as np
import pytest

import hp_adjoint as ha
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
PARITY_BOUND = 1.3e-11        # 100 x the largest relative error measured against the oracle, 1.3e-13 (ceiling 1e-9)


def _make(E, N, Ng, seed=1, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    X = np.empty((E, N))
    V = np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=seed + 7 * e)
    env.reset(X, V)
    env.set_actuator(oc.E_field(L, Ng, M))
    return env, X, V


def _actions(T, E, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (T, E, 2 * M))


def _ext_of(actions, Ng):
    T, E, _ = actions.shape
    out = np.empty((T, E, Ng))
    for t in range(T):
        for e in range(E):
            out[t, e] = po.actuator_field(L, Ng, M, actions[t, e, :M], actions[t, e, M:]).ravel()
    return out


def _bt(g_ext, Ng):
    bc, bs = po.actuator_basis(L, Ng, M)
    return np.concatenate([g_ext @ bc, g_ext @ bs], axis=-1)


def _taped_grad(env, actions, cot_hist, cot_x=None, cot_v=None, every=0):
    env.start_tape(actions.shape[0], every)
    env.step_actions_traj(actions)
    T, E = actions.shape[:2]
    out = env._h.tape_backward(cot_hist, cot_x, cot_v, ext=True, actions=True, particles=True)
    st = env.tape_stats()
    env.stop_tape()
    assert st["replay_mismatches"] == 0, st
    assert st["unit_retries"] == 0, st
    return out


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


@pytest.mark.parametrize("E,N,Ng,Ts", [(4, 3000, 64, (1, 5, 20)), (2, 20000, 250, (5, 20)), (1, 40000, 128, (5,))])
def test_adjoint_matches_autograd(E, N, Ng, Ts):
    for T in Ts:
        env, X, V = _make(E, N, Ng, seed=T)
        x0, v0 = env.particles()
        rng = np.random.default_rng(T)
        a = _actions(T, E, T)
        cot = rng.standard_normal((T, 3, E))
        cx, cv = rng.standard_normal((E, N)), rng.standard_normal((E, N))
        out = _taped_grad(env, a, cot, cx, cv)
        S = ha.Setup(N, Ng, L, 1.0, env.dt)
        ext = _ext_of(a, Ng)
        worst = 0.0
        for e in range(E):
            ge, gx, gv = ha.autograd_vjp(x0[e], v0[e], ext[:, e], S, cot[:, :, e], cx[e], cv[e])
            errs = (_rel(out["g_ext"][:, e], ge), _rel(out["g_actions"][:, e], _bt(ge, Ng)), _rel(out["g_x0"][e], gx),
                    _rel(out["g_v0"][e], gv))
            worst = max(worst, *errs)
        record_measure(f"adjoint.parity.E{E}_N{N}_Ng{Ng}_T{T}", worst)
        assert worst < PARITY_BOUND, worst
        env.close()


def _cost(env, X, V, a, lam):
    env.reset(X, V)
    _, _, per = env.step_actions_traj(a, history=True)
    return per.sum(axis=0) + lam * (a ** 2).sum(axis=(0, 2)) * L / 4


def _cost_grad(env, X, V, a, lam):
    env.reset(X, V)
    T, E = a.shape[:2]
    cot = np.zeros((T, 3, E))
    cot[:, 2] = 1.0
    out = _taped_grad(env, a, cot)
    return out["g_actions"] + lam * a * L / 2


def test_directional_derivative_matches_device_finite_differences():
    E, N, Ng, T, lam = 2, 5000, 64, 10, 0.1
    env, X, V = _make(E, N, Ng, seed=3)
    a = _actions(T, E, 3)
    g = _cost_grad(env, X, V, a, lam)
    rng = np.random.default_rng(9)
    eps = 1e-6
    worst = 0.0
    for _ in range(3):
        d = rng.standard_normal(a.shape)
        fd = (_cost(env, X, V, a + eps * d, lam).sum() - _cost(env, X, V, a - eps * d, lam).sum()) / (2 * eps)
        an = float((g * d).sum())
        worst = max(worst, abs(fd - an) / abs(an))
    record_measure("adjoint.fd_rel_eps1e-6", worst)
    assert worst < 1.5e-7, worst         # 100 x the 1.5e-9 measured at eps = 1e-6 (ceiling 1e-5)
    env.close()


def test_one_gradient_step_lowers_the_cost_in_every_environment():
    E, N, Ng, T, lam = 4, 5000, 250, 20, 0.1
    env, X, V = _make(E, N, Ng, seed=5)
    a = _actions(T, E, 5)
    J0 = _cost(env, X, V, a, lam)
    g = _cost_grad(env, X, V, a, lam)
    eta = 1e-3 * J0 / (g ** 2).sum(axis=(0, 2))
    J1 = _cost(env, X, V, a - eta[None, :, None] * g, lam)
    assert np.all(J1 < J0), (J0, J1)
    env.close()


def test_gradients_are_bitwise_reproducible():
    E, N, Ng, T = 3, 3000, 64, 7
    a = _actions(T, E, 2)
    rng = np.random.default_rng(2)
    cot = rng.standard_normal((T, 3, E))
    cx, cv = rng.standard_normal((E, N)), rng.standard_normal((E, N))

    def run(every=0, **kw):
        env, X, V = _make(E, N, Ng, seed=2, **kw)
        out = _taped_grad(env, a, cot, cx, cv, every)
        sched = env._h.schedule()
        env.close()
        return out, sched

    ref, s0 = run()
    variants = [run()[0], run(blocks_per_env=1)[0], run(blocks_per_env=2)[0], run(blocks_per_env=-1)[0]]
    variants += [run(every=k)[0] for k in (1, 3, T)]
    assert s0 == "resident" and run(blocks_per_env=2)[1] == "streaming"
    for out in variants:
        for k in ref:
            assert np.array_equal(out[k], ref[k]), k
    # environment 1 alone
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    x1, v1 = po.synthetic_bump_on_tail(N, L, seed=2 + 7)
    one = BatchedPIC(1, N, Ng, L=L, dt=0.1)
    one.reset(np.asarray(x1)[None], np.asarray(v1)[None])
    one.set_actuator(oc.E_field(L, Ng, M))
    alone = _taped_grad(one, a[:, 1:2], cot[:, :, 1:2], cx[1:2], cv[1:2])
    for k in ("g_ext", "g_actions"):
        assert np.array_equal(alone[k][:, 0], ref[k][:, 1]), k
    for k in ("g_x0", "g_v0"):
        assert np.array_equal(alone[k][0], ref[k][1]), k
    one.close()


@pytest.mark.parametrize("blocks", [0, 2])
def test_taping_does_not_perturb_the_forward(blocks):
    E, N, Ng, T = 2, 3000, 64, 6
    a = _actions(T, E, 4)
    envs = [_make(E, N, Ng, seed=4, blocks_per_env=blocks)[0] for _ in range(2)]
    taped, twin = envs
    for env in envs:
        env._h.record_start(stride=2, n_modes=2, x_bins=8, capacity=16)
    taped.start_tape(T + 3, 2)
    h1 = taped.step_actions_traj(a, history=True)
    h2 = twin.step_actions_traj(a, history=True)
    for u, w in zip(h1, h2):
        assert np.array_equal(u, w)
    for u, w in zip(taped.particles() + taped.fields() + taped.energies(), twin.particles() + twin.fields() + twin.energies()):
        assert np.array_equal(u, w)
    taped.backward(d_PE_reward=np.ones((T, E)))
    for u, w in zip(taped.particles() + taped.fields() + taped.energies(), twin.particles() + twin.fields() + twin.energies()):
        assert np.array_equal(u, w)
    # the handle keeps stepping like the twin
    for env in envs:
        env.step_actions(a[0], 3)
    for u, w in zip(taped.particles() + taped.fields() + taped.energies(), twin.particles() + twin.fields() + twin.energies()):
        assert np.array_equal(u, w)
    # same sweep grid and the same cut points (tape interval = recorder stride): every record equal, KE included
    r1, r2 = taped._h.record_read(), twin._h.record_read()
    for k in r1:
        assert np.array_equal(np.asarray(r1[k]), np.asarray(r2[k]), equal_nan=True), k
    taped.stop_tape()
    for env in envs:
        env.close()


def test_tape_contract():
    from ocplasma_amd._abi import PicError
    env, X, V = _make(1, 2000, 64, seed=6)
    env.start_tape(4, 2)
    refused = [lambda: env.step_feedback(1), lambda: env._h.step_stage(1), lambda: env.reset(X, V),
               lambda: env.reset_sampled("two-stream"), lambda: env._h.set_particles(X, V),
               lambda: env._h.set_actuator(np.zeros((64, 2)), np.zeros((64, 2))),
               lambda: env._h.set_integrator("verlet")]
    for f in refused:
        with pytest.raises(PicError, match="-3"):
            f()
    x_before = env.particles()[0].copy()
    with pytest.raises(PicError, match="-4"):
        env.step(None, 5)                                            # past max_steps: refused before any step
    assert np.array_equal(env.particles()[0], x_before)
    env.step(None, 4)
    assert env.tape_stats()["steps"] == 4
    with pytest.raises(PicError, match="-3"):
        env.start_tape(2)
    env.stop_tape()
    with pytest.raises(PicError, match="-4"):
        env.start_tape(10 ** 6, 1, budget_bytes=1 << 20)
    with pytest.raises(PicError, match="-4"):
        env.start_tape(1 << 40)
    env.close()
    for kw, what in (({"dtype": "float32"}, "float64"), ({"accum_dtype": "float64"}, "order"), ({"interpol": "TSC"}, "TSC")):
        from ocplasma_amd.env.batched import BatchedPIC
        e2 = BatchedPIC(1, 2000, 64, L=L, dt=0.1, **kw)
        e2.reset_sampled("two-stream")
        with pytest.raises(PicError, match=what):
            e2.start_tape(3)
        e2.close()
    from ocplasma_amd.env.batched import BatchedPIC
    e3 = BatchedPIC(1, 2000, 64, L=L, dt=0.1, integrator="verlet")
    e3.reset_sampled("two-stream")
    with pytest.raises(PicError, match="Yoshida"):
        e3.start_tape(3)
    e3.close()


@pytest.mark.parametrize("E", [2, 6])
def test_adjoint_matches_autograd_for_every_kind_of_control(E):
    """Raw fields (a trajectory, and one held by pic_step / step_observe), held actions given on the host (E = 2: inside the
    kernel arguments; E = 6: staged to the device), held actions on the device and step_observe's action: every way a step's
    e_t reaches the tape, against the oracle."""
    import torch
    N, Ng = 3000, 64
    env, X, V = _make(E, N, Ng, seed=20 + E)
    x0, v0 = env.particles()
    rng = np.random.default_rng(E)
    raw = 0.05 * rng.standard_normal((5, E, Ng))
    acts = _actions(3, E, E)
    T = 9
    env.start_tape(T, 3)
    env.step_ext_traj(raw[0:2])                                     # t = 0, 1
    env.step(raw[2], 2)                                             # t = 2, 3 (held field)
    env.step_actions(acts[0], 2)                                    # t = 4, 5 (held host action)
    env.step_actions_torch(torch.tensor(acts[1], dtype=torch.float64, device="cuda"))   # t = 6 (device action)
    env.step_observe(actions=acts[2])                               # t = 7
    env.step_observe(E_external=raw[3])                             # t = 8
    ext = np.concatenate([raw[0:2], raw[2:3], raw[2:3], _ext_of(acts[[0, 0, 1, 2]], Ng), raw[3:4]])
    cot = rng.standard_normal((T, 3, E))
    cx, cv = rng.standard_normal((E, N)), rng.standard_normal((E, N))
    out = env._h.tape_backward(cot, cx, cv, ext=True, actions=False, particles=True)
    st = env.tape_stats()
    env.stop_tape()
    assert st["steps"] == T and st["replay_mismatches"] == 0 and st["replay_bad_positions"] == 0, st
    S = ha.Setup(N, Ng, L, 1.0, env.dt)
    worst = 0.0
    for e in range(E):
        ge, gx, gv = ha.autograd_vjp(x0[e], v0[e], ext[:, e], S, cot[:, :, e], cx[e], cv[e])
        worst = max(worst, _rel(out["g_ext"][:, e], ge), _rel(out["g_x0"][e], gx), _rel(out["g_v0"][e], gv))
    record_measure(f"adjoint.parity.controls_E{E}", worst)
    assert worst < PARITY_BOUND, worst
    env.close()


def test_backward_refuses_a_replay_that_left_the_forward():
    """Particles written through the device views while taping: the replay no longer reproduces the forward, and the gradient
    is refused instead of returned."""
    from ocplasma_amd._abi import PicError
    env, X, V = _make(2, 3000, 64, seed=12)
    a = _actions(4, 2, 12)
    env.start_tape(4)
    env.step_actions_traj(a)
    env.sync()
    import torch
    env.torch_views()["x"][0, 10] += 1e-3
    torch.cuda.synchronize()
    with pytest.raises(PicError, match="replay differs"):
        env.backward(d_PE_reward=np.ones((4, 2)))
    assert env.tape_stats()["replay_mismatches"] > 0
    env.stop_tape()
    env.close()


def test_default_interval_follows_the_budget():
    """checkpoint_every = 0: ceil(sqrt(T)) when the budget allows it, else the interval needing the fewest bytes."""
    from ocplasma_amd._abi import PicError
    env, X, V = _make(2, 3000, 64, seed=13)
    T = 16
    sizes = {}
    for k in range(1, T + 1):
        env.start_tape(T, k)
        sizes[k] = env.tape_stats()["bytes"]
        env.stop_tape()
    best = min(sizes, key=lambda k: (sizes[k], k))
    env.start_tape(T)
    assert env.tape_stats()["checkpoint_every"] == 4
    env.stop_tape()
    assert sizes[best] < sizes[4], sizes
    env.start_tape(T, 0, budget_bytes=sizes[best])
    st = env.tape_stats()
    assert st["checkpoint_every"] == best and st["bytes"] == sizes[best], st
    env.stop_tape()
    with pytest.raises(PicError, match="-4"):
        env.start_tape(T, 0, budget_bytes=sizes[best] - 1)
    env.close()


# (bytes, checkpoint_every, launches) of pic_tape_stats after every action of _accounting below, from the code as it was before the
# tape's device blocks were described by one carver (csrc/host_diff.h): worked out by hand from that code's layout functions
# (every part rounded up to 256 bytes; ld = 1024; the law's last part unrounded) and its launch counters, not from the carver.
# Byte accounting is behaviour: these are never re-recorded from the code under test.
ACCOUNTING = {
    "start_every0": (254976, 3, 0),
    "start_every1": (312320, 1, 0),
    "start_every2": (250880, 2, 0),
    "start_every5": (328704, 5, 0),
    "kl_shared": (253952, 2, 0),                  # + 3072: feq 512, acc 1024, g 1024, trace 80 -> 256, cot 256
    "kl_per_env": (254464, 2, 0),                 # + 3584: feq 1024
    "gain": (257280, 2, 0),                       # + 3 x 512 + 1024 (the law's record) + 256 (the gain)
    "backward": (257280, 2, 50),                  # replay 17, steps 14 + 15 (KL 3, the law's E-bar 0 + 1, 11), close 3, a-bar 1
    "tangent_K1": (286208, 2, 40),                # + 35328; start 1, replay 17, 2 x 11
    "tangent_K5": (425472, 2, 40),                # + 174592
}


def _accounting_env():
    """2 environments, N = 1000, 64 nodes, two actuator modes: a row of actions is 64 bytes and a mesh 512, shorter than the 256
    bytes every part of a block is rounded up to."""
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    E, N, Ng = 2, 1000, 64
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    X, V = np.empty((E, N)), np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=31 + 7 * e)
    env.reset(X, V)
    env.set_actuator(oc.E_field(L, Ng, 2))
    return env, X, V


def _accounting(env, X, V, budget=None, only=None):
    """name -> (bytes, checkpoint_every, launches) after every action, max_steps = 5 throughout.  Tapes with checkpoint_every 0
    (= 3), 1, 2 and 5; then, each on a tape of its own with checkpoint_every = 2: a KL of 8 x 8 bins with a shared target; one
    with a target per environment; that, one gain-law call of 2 steps and a backward over them with energy and KL cotangents;
    two plain steps and the tangent for K = 1; those and then K = 5 (pic_tape_tangent refuses a tape that holds gain-law steps,
    so the tangents have tapes of their own).  budget: name -> budget_bytes of the tape that ends with that action (none by
    default); only: the tapes to make (all by default)."""
    budget = budget or {}
    E, Mk, T = env.num_envs, 2, 5
    h = env._h
    got = {}

    def note(name):
        st = env.tape_stats()
        got[name] = (st["bytes"], st["checkpoint_every"], st["launches"])

    def tape(name, every=2):
        if only is not None and name not in only:
            return False
        env.stop_tape()
        env.reset(X, V)
        env.start_tape(T, every, budget_bytes=budget.get(name, 0))
        return True

    feq = np.random.default_rng(32).uniform(0.0, 2.0 / (L * 12.0), (E, 8, 8))
    ones = np.ones((2, E))
    acts = np.random.default_rng(33).uniform(-0.5, 0.5, (2, E, 2 * Mk))
    for every in (0, 1, 2, 5):
        if tape(f"start_every{every}", every):
            note(f"start_every{every}")
    if tape("kl_shared"):
        h.tape_kl_start(8, 8, -6.0, 6.0, feq[0].ctypes.data, 0, 0)
        note("kl_shared")
    if tape("kl_per_env"):
        h.tape_kl_start(8, 8, -6.0, 6.0, feq.ctypes.data, 1, 0)
        note("kl_per_env")
    if tape("gain"):
        h.tape_kl_start(8, 8, -6.0, 6.0, feq.ctypes.data, 1, 0)
        env.step_feedback_gain(0.1 * np.eye(2 * Mk), 2)
        note("gain")
        h.tape_kl_cot(ones.ctypes.data, 0, 0, 2)
        h.tape_backward_feedback(cot_hist=np.ones((2, 3, E)))
        note("backward")
    for name, Ks in (("tangent_K1", (1,)), ("tangent_K5", (1, 5))):
        if tape(name):
            env.step_actions_traj(acts)
            for K in Ks:
                h.tape_tangent(K, d_actions=np.ones((K, 2, E, 2 * Mk)))
            note(name)
    env.stop_tape()
    return got


def test_tape_byte_accounting_is_pinned():
    """Absolute values of pic_tape_stats' bytes, checkpoint_every and launches (ACCOUNTING), and budget_bytes to the byte: the
    recorded total is accepted, one byte less is refused with PIC_ENOMEM by the very entry that needs it.  (With
    checkpoint_every = 0 one byte less than the total of the default interval 3 is not a refusal: the tape then takes the
    interval that needs the fewest bytes, 2, and it is one byte below that total that is refused.)"""
    from ocplasma_amd._abi import PicError
    env, X, V = _accounting_env()
    assert _accounting(env, X, V) == ACCOUNTING
    totals = {k: v[0] for k, v in ACCOUNTING.items() if k != "backward"}           # (a backward allocates nothing)
    assert _accounting(env, X, V, totals) == ACCOUNTING                            # exactly enough, everywhere
    got = _accounting(env, X, V, {"start_every0": totals["start_every0"] - 1}, only={"start_every0"})
    assert got == {"start_every0": ACCOUNTING["start_every2"]}
    entry = {"start": "pic_tape_start", "kl": "pic_tape_kl_start", "gain": "pic_step_feedback_gain", "tangent": "pic_tape_tangent"}
    for name in totals:
        floor = totals["start_every2" if name == "start_every0" else name]
        with pytest.raises(PicError, match=f"error -4: {entry[name.split('_')[0]]}:"):
            _accounting(env, X, V, {name: floor - 1}, only={name})
    env.close()


# The blocks ACCOUNTING does not reach, at its shape (E = 2, N = 1000, Ng = 64, two actuator modes, max_steps = 5,
# checkpoint_every = 2): name -> (bytes, checkpoint_every, launches) of pic_tape_stats behind the last action of the tape of that
# name (_more_accounting).  Recorded from a run of the code as it was before the blocks got one reserve path (csrc/host_diff.h:
# tape_reserve) and checked against the sums of that code's layout functions, which tests/test_blocks_cpu.py pins on the CPU (every
# part rounded up to 256 bytes; a row of actions is 64 bytes, of observations 96, a mesh of both environments 1024, ld = 1024).  Never re-recorded from
# the code under test.
START2, TANGENT1, TANGENT5 = 250880, 35328, 174592        # ACCOUNTING: start_every2, and what tangent_K1 / tangent_K5 add to it
MORE_ACCOUNTING = {
    # the record: o, u, a, o-bar, u-bar, a-bar and the two direct cotangents 8 x 512 (480 and 320 bytes rounded), m-bar 96 -> 256,
    # the per-environment sums 2 x 59 x 8 = 944 -> 1024, their sum 472 -> 512; a call's copy: the parameters 472 -> 512 and the 48
    # bytes of obs_scale behind them, unrounded; two calls
    "policy_shared": (START2 + 5888 + 2 * 560, 2, 0),
    "policy_per_env": (START2 + 5376 + 1072, 2, 0),       # no sum over the environments; the copy: 944 -> 1024, + 48
    # the walk's rows for K = 1 and two observed modes: dM 1024, energies 48 -> 256, observation, dm, da 64 -> 256 each, dG 256,
    # injection 1024; begin: 1 launch of the start's field, the law kernel, the start kernel
    "twalk_K1": (START2 + TANGENT1 + 3328, 2, 3),
    "twalk_K5": (START2 + TANGENT5 + 13312, 2, 3),        # dM 5120, 240 -> 256, 3 x (320 -> 512), dG 1280, injection 5120
    # the tangent's block for K = 1, the walk's rows with three observed modes (96 -> 256: as above) and the policy tangent's:
    # dtheta 472 -> 512, du 256, d_pre 256; launches: begin 3, replay 17, 2 x (policy JVP 1, step 11, law 1)
    "tpol": (START2 + 5888 + 560 + TANGENT1 + 3328 + 1024, 2, 46),
    "mom_cot": (START2 + 18432, 2, 0),                    # 6 rows of 2 x 3 x 64 doubles
    "mom_trace": (START2 + 15360, 2, 0),                  # 5 rows
    "tkl": (START2 + 3072 + TANGENT1 + 256 + 256, 2, 48), # kl_shared's block; unit cotangents 16 -> 256, 8 x 2 x 1 chunk sums 128 -> 256
    "tmom": (START2 + TANGENT1 + 24576 + 512, 2, 46),     # sums 3 x 8 x 2 x 64 words, max words 3 x 8 x 2 x 8 = 384 -> 512
}
# what the refusal of the last action leaves in `bytes` on top of what was there: tangent_policy reserves the tangent's block and
# the walk's rows before the policy tangent's, each on its own
MORE_PARTIAL = {"tpol": TANGENT1 + 3328}
MORE_ENTRY = {"policy_shared": "pic_tape_step_policy", "policy_per_env": "pic_tape_step_policy",
              "twalk_K1": "pic_tape_tangent_walk_begin", "twalk_K5": "pic_tape_tangent_walk_begin", "tpol": "pic_tape_tangent_policy",
              "mom_cot": "pic_tape_moments_cot", "mom_trace": "pic_tape_moments_start", "tkl": "pic_tape_tangent_kl",
              "tmom": "pic_tape_tangent_moments"}
# E = 1, Ng = 100 (pic_create takes any Ng >= 4): the tape, the law's record 3 x (160 -> 256) + the 800 bytes of its last part,
# unrounded, and a gain of 128 bytes (unrounded as well: an allocation of its own)
LAW_TAIL = (132352 + 3 * 256 + 800 + 128, 2, 0)


def _more_accounting(env, X, V, name, budget=0):
    """The tape `name` of MORE_ACCOUNTING with budget_bytes = budget: every action but the last, then -> (the last action as a
    callable, pic_tape_stats in front of it)."""
    from ocplasma_amd.control.policy import MLPPolicy
    E, Mk, T, Mo = env.num_envs, 2, 5, 3
    h = env._h
    env.stop_tape()
    env.reset(X, V)
    env.start_tape(T, 2, budget_bytes=budget)
    rng = np.random.default_rng(34)
    acts = rng.uniform(-0.5, 0.5, (2, E, 2 * Mk))
    widths = (2 * Mo, 5, 2 * Mk)
    P = sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(2))           # 59

    def policy(per_env):
        theta = rng.uniform(-0.3, 0.3, (E, P) if per_env else (P,))
        return MLPPolicy(widths, "tanh", theta, Mo, squash=True, obs_scale=np.ones(2 * Mo), per_env=per_env)

    if name == "policy_shared":
        pol = policy(False)
        env.tape_step_policy(pol, 1)
        last = lambda: env.tape_step_policy(pol, 1)
    elif name == "policy_per_env":
        last = lambda pol=policy(True): env.tape_step_policy(pol, 2)
    elif name in ("twalk_K1", "twalk_K5"):
        env.step_actions_traj(acts)
        h.tape_tangent(1, d_actions=np.ones((1, 2, E, 2 * Mk)))
        last = lambda: env.tangent_walk(K=1)
        if name == "twalk_K5":
            last()
            h.tape_tangent(5, d_actions=np.ones((5, 2, E, 2 * Mk)))
            last = lambda: env.tangent_walk(K=5)
    elif name == "tpol":
        pol = policy(False)
        env.tape_step_policy(pol, 2)
        last = lambda: env.tangent_policy(d_params=np.ones(P))
    elif name == "mom_cot":
        env.step_actions_traj(acts)
        cot = np.ones((2, E, 3, 64))
        last = lambda: h.tape_moments_cot(cot.ctypes.data, 0, 0, 2)
    elif name == "mom_trace":
        last = h.tape_moments_start
    elif name == "tkl":
        feq = np.random.default_rng(32).uniform(0.0, 2.0 / (L * 12.0), (8, 8))
        h.tape_kl_start(8, 8, -6.0, 6.0, feq.ctypes.data, 0, 0)
        env._tape_kl = True
        env.step_actions_traj(acts)
        env.tangent(d_actions=np.ones((2, E, 2 * Mk)))
        last = lambda: env.tangent(d_actions=np.ones((2, E, 2 * Mk)), kl=True)
    elif name == "tmom":
        env.step_actions_traj(acts)
        env.tangent(d_actions=np.ones((2, E, 2 * Mk)))
        last = lambda: env.tangent(d_actions=np.ones((2, E, 2 * Mk)), moments=True)
    else:
        raise KeyError(name)
    return last, env.tape_stats()


def _stats3(env):
    st = env.tape_stats()
    return st["bytes"], st["checkpoint_every"], st["launches"]


def test_tape_byte_accounting_of_the_attached_blocks_is_pinned():
    """MORE_ACCOUNTING: the policy's record and its per-call copies, the tangent walk's rows and their growth, the policy
    tangent's rows, the moments' cotangents and trace, and the blocks behind the KL's and the moments' tangents.  For each: the
    recorded total without a budget, the same total accepted as budget_bytes to the byte, and one byte less refused with
    PIC_ENOMEM by the entry that needs the block, with steps and bytes as they were -- twice, where the entry reserves other
    blocks first (MORE_PARTIAL)."""
    from ocplasma_amd._abi import PicError
    env, X, V = _accounting_env()
    for name, want in MORE_ACCOUNTING.items():
        for budget in (0, want[0]):
            last, _ = _more_accounting(env, X, V, name, budget)
            last()
            got = _stats3(env)
            print(name, budget, got)
            assert got == want, (name, budget, got)
        last, before = _more_accounting(env, X, V, name, want[0] - 1)
        held = before["bytes"] + MORE_PARTIAL.get(name, 0)
        for _ in range(2):
            with pytest.raises(PicError, match=f"error -4: {MORE_ENTRY[name]}:"):
                last()
            st = env.tape_stats()
            assert (st["steps"], st["bytes"]) == (before["steps"], held), (name, st, before)
    env.stop_tape()
    env.close()


def test_tape_byte_accounting_keeps_the_laws_unrounded_tail():
    """LAW_TAIL: at E = 1, Ng = 100 the last part of the law's record, E-bar [env][Ng], takes its 800 bytes, not 1024."""
    import ocplasma_amd as oc
    from ocplasma_amd._abi import PicError
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(1, 1000, 100, L=L, dt=0.1)
    X, V = (a[None] for a in po.synthetic_bump_on_tail(1000, L, seed=31))
    env.reset(X, V)
    env.set_actuator(oc.E_field(L, 100, 2))
    for budget in (0, LAW_TAIL[0]):
        env.start_tape(5, 2, budget_bytes=budget)
        env.step_feedback_gain(0.1 * np.eye(4), 2)
        got = _stats3(env)
        print("law_tail", budget, got)
        assert got == LAW_TAIL, (budget, got)
        env.stop_tape()
        env.reset(X, V)
    env.start_tape(5, 2, budget_bytes=LAW_TAIL[0] - 1)
    before = env.tape_stats()
    with pytest.raises(PicError, match="error -4: pic_step_feedback_gain:"):
        env.step_feedback_gain(0.1 * np.eye(4), 2)
    st = env.tape_stats()
    assert (st["steps"], st["bytes"]) == (before["steps"], before["bytes"]), (st, before)
    env.stop_tape()
    env.close()


def test_torch_rollout_matches_tape_and_passes_gradcheck():
    import torch
    from ocplasma_amd._abi import PicError
    from ocplasma_amd.env import grad
    E, N, Ng, T = 2, 3000, 64, 5
    env, X, V = _make(E, N, Ng, seed=8)
    a = _actions(T, E, 8)
    at = torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    ke, pe, per = grad.rollout(env, at)
    (per.sum() + 0.5 * ke.sum()).backward()
    env.stop_tape()
    env.reset(X, V)
    cot = np.zeros((T, 3, E))
    cot[:, 2] = 1.0
    cot[:, 0] = 0.5
    ref = _taped_grad(env, a, cot)
    assert np.array_equal(at.grad.cpu().numpy(), ref["g_actions"])
    # a stale backward raises
    env.reset(X, V)
    at2 = torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    ke, pe, per = grad.rollout(env, at2)
    with pytest.raises(PicError, match="-4"):
        env.step_actions(a[0])                                       # the rollout's tape is full: no step can slip in
    env.stop_tape()
    env.reset(X, V)                                                  # the environment moves on
    with pytest.raises(PicError, match="moved on"):
        per.sum().backward()
    env.stop_tape()
    env.close()
    # gradcheck at 2 x N = 500, T = 3: every evaluation on an environment of its own (gradcheck evaluates the function again
    # between the forward and the backward it checks, which would make a shared environment's tape stale)
    def f(u):
        env, _, _ = _make(2, 500, 32, seed=9)
        return grad.rollout(env, u)
    u = torch.tensor(_actions(3, 2, 9), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(f, (u,), eps=1e-6, atol=1e-6, rtol=1e-4)
    # raw fields: rollout_ext against the tape of step_ext_traj
    env, X, V = _make(2, 3000, 64, seed=14)
    e = 0.05 * np.random.default_rng(14).standard_normal((4, 2, 64))
    et = torch.tensor(e, dtype=torch.float64, device="cuda", requires_grad=True)
    ke, pe, per = grad.rollout_ext(env, et)
    (pe.sum() - ke.sum()).backward()
    env.stop_tape()
    env.reset(X, V)
    cot = np.zeros((4, 3, 2))
    cot[:, 1] = 1.0
    cot[:, 0] = -1.0
    env.start_tape(4)
    env.step_ext_traj(e)
    ref = env._h.tape_backward(cot)
    env.stop_tape()
    assert np.array_equal(et.grad.cpu().numpy(), ref["g_ext"])
    env.close()
