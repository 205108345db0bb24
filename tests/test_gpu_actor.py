"""The DeepSets particle actor on the device (pic_actor_eval, pic_step_actor): the head against the NumPy
restatement of its arithmetic (tests/hp_actor.py), the three sources of the features against `pool` bit for bit, whole rollouts
against the host loop pool -> actor_eval(features) -> step_actions they replace (on both schedules, in host and in device
memory), the reference's actor (g20), batch independence, the NaN rule, interleaved calls on one handle, the C contract and the
torch twin."""
import ctypes

import numpy as np
import pytest

import hp_actor as ha
import hp_pool as hp
import hp_pool_ln as hl
from conftest import record_measure

pytestmark = pytest.mark.gpu

L = 50.0
EINVAL, ESTATE = -1, -3


def _make(E, N, Ng=32, M=2, reset=None, actuator=True, dtype="float64", seed=1, **kw):
    """An environment of E x N particles; reset: None = box_data's particles, False = no reset."""
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, dtype=dtype, **kw)
    if reset is None:
        X, V = hp.box_data(E, N, seed=seed)
        X = X.astype(dtype)
        X[X >= L] = 0.0                                     # (the last double below L rounds to L in float32)
        env.reset(X, V.astype(dtype))
    if actuator:
        env.set_actuator(oc.E_field(L, Ng, M))
    return env


def _actor(H, head, layernorm, activation, M, pool_ln, seed=0, lead=(), squash=True, params=None, v_scale=0.25, pool_activation=None):
    """`activation` is the head's; the per-particle layer has pool_activation (None: the same)."""
    from ocplasma_amd.control.actor import ParticleActor
    widths = ha.stacks(H, M)[head]
    W, b, g, be = hl.layer(H, seed + 1, lead) if pool_ln else hp.layer(H, seed + 1, lead) + (None, None)
    params = ha.make_params(widths, layernorm, seed + 2, lead) if params is None else params
    return ParticleActor(W, b, widths, params, pool_activation or activation, gamma=g, beta=be, v_scale=v_scale, layernorm=layernorm,
                         squash=squash, action_scale=1.25 if squash else 1.0, action_shift=0.75 if squash else 0.0, per_env=bool(lead),
                         head_activation=activation)


def _pool(env, actor, x=None, v=None, on_device=False):
    return env.pool(actor.W, actor.b, actor.activation, actor.v_scale, x=x, v=v, on_device=on_device, gamma=actor.gamma, beta=actor.beta,
                    eps=actor.eps, period=actor.period)


def _state(env):
    return [np.asarray(a).copy() for a in (*env.particles(), *env.fields(), *env.energies())]


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _cuda(*arrays):
    import torch
    return [None if a is None else torch.as_tensor(a, device="cuda") for a in arrays]


def _on_device(actor):
    """The actor with its head's parameters in device memory: its calls then work in device memory."""
    return actor.with_params(_cuda(_np(actor.params))[0])


OTHER = {"tanh": "relu", "relu": "tanh"}


# ---- 1. the head against the restatement ----------------------------------------------------------------------------------------
def test_actor_eval_on_features_against_the_restatement():
    """pre, and actions relative to max(1, |action_scale| + |action_shift|), within 100 x the largest float64 - longdouble
    difference of the restatement over these cases (1.08e-15 -> 1.08e-13): a quantity of the references alone.  The device's
    tanh and NumPy's may differ in the last bits."""
    bound = 100 * ha.eval_floor()
    envs, worst = {}, 0.0
    for i, case in enumerate(ha.EVAL_CASES):
        E, H, head, layernorm, activation, per_env, M, squash = case
        c = ha.eval_case(*case)
        if (E, M) not in envs:
            envs[E, M] = _make(E, 63, M=M, reset=False)
        env = envs[E, M]
        # (the per-particle layer has the other activation: the head must take its own)
        actor = _actor(H, head, layernorm, activation, M, pool_ln=bool(i % 2), lead=(E,) if per_env else (), squash=squash, params=c["params"],
                       pool_activation=OTHER[activation])
        want_u, want_a = ha.forward(**c)
        for dev in (False, True):
            a = _on_device(actor) if dev else actor
            f, u, act = env.actor_eval(a, features=c["features"], noise=c["noise"], std=c["std"])
            assert hasattr(u, "is_cuda") == dev and np.array_equal(_np(f), c["features"])
            eu = float(np.max(np.abs(_np(u) - want_u)))
            ea = float(np.max(np.abs(_np(act) - want_a))) / ha.action_unit(c)
            print(f"actor_eval {case}: pre {eu:.3g} actions {ea:.3g} bound {bound:.3g}")
            assert eu <= bound and ea <= bound, case
            worst = max(worst, eu, ea)
        # without noise pre is z
        _, u0, _ = env.actor_eval(actor, features=c["features"])
        c0 = dict(c, noise=None, std=None)
        assert float(np.max(np.abs(u0 - ha.forward(**c0)[0]))) <= bound
    for env in envs.values():
        env.close()
    record_measure("actor_eval_err", worst)


# ---- 2. the three sources of the features ---------------------------------------------------------------------------------------
SOURCES = (
    # E, N, H, head, layernorm, activation, per_env, M, pool_ln
    (1, 1, 1, 0, True, "relu", False, 1, True),
    (3, 1, 5, 1, True, "tanh", True, 3, False),
    (3, 63, 64, 1, True, "relu", False, 1, True),
    (1, 63, 256, 0, False, "tanh", False, 3, False),
    (3, 1025, 5, 2, True, "relu", True, 1, True),
    (1, 1025, 64, 0, False, "relu", False, 3, True),
    (3, 1025, 256, 1, False, "tanh", False, 3, False),
)


@pytest.mark.parametrize("case", SOURCES, ids=lambda c: "-".join(map(str, c)))
def test_features_are_pools_and_the_head_is_the_heads(case):
    E, N, H, head, layernorm, activation, per_env, M, pool_ln = case
    # (every second case with another activation in the per-particle layer than in the head: `pool` takes the former)
    actor = _actor(H, head, layernorm, activation, M, pool_ln, seed=N, lead=(E,) if per_env else (),
                   pool_activation=OTHER[activation] if E == 3 else None)
    rng = np.random.default_rng(N + H)
    eps, std = rng.normal(size=(E, 2 * M)), rng.uniform(0.05, 0.3, 2 * M)
    env = _make(E, N, M=M, seed=5)                          # (the stored particles: box_data, wrapped)
    X, V = hp.box_data(E, N, seed=6)
    X = X + L * rng.integers(-1, 3, size=X.shape)           # positions partly outside [0, L)
    before = _state(env)
    for x, v in ((X, V), (None, None)):
        feats = _pool(env, actor, x, v)
        f, u, a = env.actor_eval(actor, x=x, v=v, noise=eps, std=std)
        assert np.array_equal(f, feats, equal_nan=True) and np.isfinite(f).all()
        f2, u2, a2 = env.actor_eval(actor, features=feats, noise=eps, std=std)
        assert np.array_equal(u, u2) and np.array_equal(a, a2) and np.array_equal(f2, feats)
        # device memory gives the same bits
        xd, vd, ed, sd = _cuda(x, v, eps, std)
        fd, ud, ad = env.actor_eval(_on_device(actor), x=xd, v=vd, noise=ed, std=sd)
        assert fd.is_cuda and np.array_equal(_np(fd), f) and np.array_equal(_np(ud), u) and np.array_equal(_np(ad), a)
    assert _same(_state(env), before)                       # the state is not touched
    env.close()


# ---- 3. a rollout is the host loop ----------------------------------------------------------------------------------------------
T6, E3, N3, NG3, M3, H3 = 6, 3, 1025, 64, 2, 5
_LOOPS = {}
VARIANTS = {"plain": dict(), "tsc": dict(interpol="TSC"), "verlet": dict(integrator="verlet"), "recorder": dict()}


def _rollout_actor(per_env=False, pool_ln=True):
    # (the deep head: behind the width-1 layer of the middle one a LayerNorm leaves beta alone, and the actions would be constants)
    return _actor(H3, 2, True, "relu", M3, pool_ln, seed=3, lead=(E3,) if per_env else ())


def _noise(T=T6, E=E3):
    rng = np.random.default_rng(9)
    return rng.normal(size=(T, E, 2 * M3)), rng.uniform(0.05, 0.3, 2 * M3)


def _start(env, variant):
    if variant == "recorder":
        env.start_recording(stride=2, modes=4, x_bins=16)
    return env


def _host_loop(env, actor, T, eps=None, std=None):
    """T x (pool -> actor_eval on its features -> step_actions, all on the device); the per-step records and the final state."""
    feats, pre, act, en = [], [], [], []
    for t in range(T):
        f = _pool(env, actor, on_device=True)
        _, u, a = env.actor_eval(actor, features=f, noise=None if eps is None else eps[t], std=std, on_device=True)
        env.step_actions_torch(a)
        feats.append(_np(f)), pre.append(_np(u)), act.append(_np(a)), en.append(env.energies())
    en = np.stack([np.stack(e) for e in en])                           # [T, 3, E]
    return dict(features=np.stack(feats), pre=np.stack(pre), actions=np.stack(act), KE=en[:, 0], PE=en[:, 1], PE_reward=en[:, 2],
                state=_state(env))


def _loop(bpe, noise=True):
    """The reference loop of a schedule, computed once and shared."""
    if (bpe, noise) not in _LOOPS:
        env = _make(E3, N3, NG3, M3, blocks_per_env=bpe)
        assert env._h.schedule() == ("resident" if bpe < 0 else "streaming")
        eps, std = _noise() if noise else (None, None)
        _LOOPS[bpe, noise] = _host_loop(env, _rollout_actor(), T6 if noise else 3, eps, std)
        env.close()
    return _LOOPS[bpe, noise]


def _assert_rollout(r, ref, sl=slice(None)):
    for k in ("features", "pre", "actions", "KE", "PE", "PE_reward"):
        assert np.array_equal(_np(getattr(r, k)), ref[k][sl]), k


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("bpe", [-1, 4])
def test_step_actor_is_the_host_loop(bpe, memory):
    ref = _loop(bpe)
    eps, std = _noise()
    actor = _rollout_actor()
    if memory == "device":
        eps, std = _cuda(eps, std)
        actor = _on_device(actor)
    env = _make(E3, N3, NG3, M3, blocks_per_env=bpe)
    r = env.step_actor(actor, T6, noise=eps, std=std)
    assert (memory == "device") == hasattr(r.actions, "is_cuda")
    _assert_rollout(r, ref)
    assert _same(_state(env), ref["state"]) and env.bad_count() == 0
    env.close()
    # one call of 6 steps equals two calls of 3 steps (the second without the energies' record: the asynchronous form)
    env = _make(E3, N3, NG3, M3, blocks_per_env=bpe)
    r1 = env.step_actor(actor, 3, noise=eps[:3], std=std)
    r2 = env.step_actor(actor, 3, noise=eps[3:], std=std, history=False)
    env.sync()
    _assert_rollout(r1, ref, slice(0, 3))
    assert r2.KE is None
    for k in ("features", "pre", "actions"):
        assert np.array_equal(_np(getattr(r2, k)), ref[k][3:]), k
    assert _same(_state(env), ref["state"])
    # ... and without noise
    ref0 = _loop(bpe, noise=False)
    env.close()
    env = _make(E3, N3, NG3, M3, blocks_per_env=bpe)
    _assert_rollout(env.step_actor(actor, 3), ref0)
    assert _same(_state(env), ref0["state"])
    env.close()


@pytest.mark.parametrize("variant,bpe", [("tsc", 4), ("verlet", -1), ("recorder", 4), ("plain", -1)])
def test_step_actor_wherever_step_actions_runs(variant, bpe):
    """TSC, Verlet and the recorder once each, under a per-environment actor on the plain pool."""
    T = 3
    actor = _rollout_actor(per_env=True, pool_ln=False)
    eps, std = _noise(T)
    a, b = (_start(_make(E3, N3, NG3, M3, blocks_per_env=bpe, **VARIANTS[variant]), variant) for _ in range(2))
    ref = _host_loop(b, actor, T, eps, std)
    r = a.step_actor(actor, T, noise=eps, std=std)
    _assert_rollout(r, ref)
    assert _same(_state(a), ref["state"])
    if variant == "recorder":
        ra, rb = a.recorded(), b.recorded()
        assert len(ra) == len(rb) == 1
        for k in ("steps", "KE", "PE", "PE_reward", "field_energy", "Ek", "x_hist"):
            assert np.array_equal(np.asarray(getattr(ra, k)), np.asarray(getattr(rb, k))), k
    a.close()
    b.close()


# ---- 4. the reference's actor ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ha.G20_CASES)
def test_g20_reference_actor(pre):
    """ParticleActor.from_reference on the fixture's particles against the reference's mu and action, within the bound
    tests/test_actor_cpu.py fixes: 100 x the restated chain's own float64 - longdouble difference over the g20 cases."""
    from ocplasma_amd.control.actor import ParticleActor
    g = ha.g20()
    bound = 100 * ha.g20_floor()
    X, V = g[f"{pre}_x"], g[f"{pre}_v"]
    actor = ParticleActor.from_reference(ha.g20_state_dict(pre), L_ref=float(g["L"]), x_norm=float(g[f"{pre}_x_norm"]),
                                         v_norm=float(g[f"{pre}_v_norm"]), output_min=float(g[f"{pre}_output_min"]),
                                         output_max=float(g[f"{pre}_output_max"]))
    env = _make(X.shape[0], X.shape[1], M=int(g[f"{pre}_M"]), reset=False)
    _, u, a = env.actor_eval(actor, x=X, v=V)
    e_mu = float(np.max(np.abs(np.tanh(u) - g[f"{pre}_mu"])))
    e_a = float(np.max(np.abs(a - g[f"{pre}_action"]))) / max(1.0, abs(actor.action_scale) + abs(actor.action_shift))
    print(f"g20 {pre}: mu {e_mu:.3g} action {e_a:.3g} bound {bound:.3g}")
    record_measure(f"actor_g20_err.{pre}", max(e_mu, e_a))
    assert e_mu <= bound and e_a <= bound
    env.close()


# ---- 5. an environment alone is its row in a batch; two runs give the same bits -------------------------------------------------
@pytest.mark.parametrize("bpe", [-1, 4])
def test_an_environment_alone_is_its_row(bpe):
    T = 3
    actor = _rollout_actor()
    eps, std = _noise(T)
    X, V = hp.box_data(E3, N3, seed=1)
    runs = []
    for _ in range(2):
        env = _make(E3, N3, NG3, M3, blocks_per_env=bpe)
        runs.append((env.step_actor(actor, T, noise=eps, std=std), _state(env)))
        env.close()
    (r, s), (r2, s2) = runs
    _assert_rollout(r2, {k: _np(getattr(r, k)) for k in r._fields})
    assert _same(s, s2)
    one = _make(1, N3, NG3, M3, reset=False, blocks_per_env=bpe)
    one.reset(X[1:2], V[1:2])
    q = one.step_actor(actor, T, noise=eps[:, 1:2], std=std)
    for k in q._fields:
        assert np.array_equal(getattr(q, k), getattr(r, k)[:, 1:2]), k
    for p, w in zip(_state(one), s):
        assert np.array_equal(p, w[1:2])
    one.close()


# ---- 6. a non-finite velocity -----------------------------------------------------------------------------------------------------
def test_an_infinite_velocity_stays_in_its_environment():
    """(A tanh head: NaN passes through it.  relu's comparison y > 0 ? y : +0.0 sends a NaN to +0, as pic_policy's does, so behind a
    relu layer only the features of the faulty environment are NaN.)"""
    actor = _actor(H3, 1, True, "tanh", M3, True, seed=3)
    eps, std = _noise(1)
    X, V = hp.box_data(E3, N3, seed=1)
    env = _make(E3, N3, NG3, M3)
    f0, u0, a0 = env.actor_eval(actor, x=X, v=V, noise=eps[0], std=std)
    Vb = V.copy()
    Vb[1, 17] = np.inf
    f, u, a = env.actor_eval(actor, x=X, v=Vb, noise=eps[0], std=std)
    for got, want in ((f, f0), (u, u0), (a, a0)):
        assert np.isnan(got[1]).all()
        assert np.array_equal(got[[0, 2]], want[[0, 2]])
    # the next call on the handle is clean: the sums and the max words were cleared
    f1, u1, a1 = env.actor_eval(actor, x=X, v=V, noise=eps[0], std=std)
    assert np.array_equal(f1, f0) and np.array_equal(u1, u0) and np.array_equal(a1, a0)
    assert np.array_equal(_pool(env, actor, X, V), f0)
    # under the reference-shaped head (relu with LayerNorms) the actions of the faulty environment are finite by the contract's
    # comparison; its features_out is NaN, so the fault stays observable, and the other environments are untouched
    relu = _rollout_actor()
    g0, w0, b0 = env.actor_eval(relu, x=X, v=V, noise=eps[0], std=std)
    g, w, b = env.actor_eval(relu, x=X, v=Vb, noise=eps[0], std=std)
    assert np.isnan(g[1]).all() and np.isfinite(b[1]).all()
    for got, want in ((g, g0), (w, w0), (b, b0)):
        assert np.array_equal(got[[0, 2]], want[[0, 2]])
    # ... and the same through the stored particles of a handle
    bad = _make(E3, N3, NG3, M3, reset=False)
    bad.reset(X, Vb)
    gs, _, bs = bad.actor_eval(relu, noise=eps[0], std=std)
    assert np.isnan(gs[1]).all() and np.isfinite(bs[1]).all() and np.array_equal(gs[[0, 2]], g0[[0, 2]]) and np.array_equal(bs[[0, 2]], b0[[0, 2]])
    bad.close()
    env.close()


# ---- 7. one handle through interleaved calls ----------------------------------------------------------------------------------------
def test_interleaved_calls_on_one_handle():
    """actor_eval, step_actor, pool, pool_vjp, policy_eval and step_policy on one handle, with H, head and memory kind changing
    between the calls: each against a fresh handle that made the earlier stepping calls alone, bit for bit."""
    import hp_mlp_policy as hm
    from ocplasma_amd.control.policy import MLPPolicy
    E, N, Ng, M = 3, 1025, 64, 2
    big = _actor(64, 2, True, "relu", M, True, seed=11)
    small = _actor(5, 0, False, "tanh", M, False, seed=12, lead=(E,))
    widths = [4, 16, 2 * M]
    pol = MLPPolicy(widths, "tanh", hm.make_params(widths, 5), 2, squash=True)
    cot = np.random.default_rng(3).normal(size=(E, 64))
    eps, std = _noise(2, E)
    X, V = hp.box_data(E, N, seed=8)

    def results(r):
        if isinstance(r, dict):
            return [_np(v) for v in r.values() if v is not None]
        return [_np(v) for v in (r if isinstance(r, tuple) else (r,)) if v is not None]

    calls = [
        ("actor_eval big", lambda e: e.actor_eval(big, noise=eps[0], std=std), False),
        ("step_actor small on the device", lambda e: e.step_actor(_on_device(small), 2, noise=_cuda(eps)[0]), True),
        ("pool", lambda e: _pool(e, big), False),
        ("actor_eval small on x, v", lambda e: e.actor_eval(small, x=X, v=V), False),
        ("pool_vjp", lambda e: e.pool_vjp(big.W, big.b, cot, "relu", big.v_scale, gamma=big.gamma, beta=big.beta), False),
        ("step_actor big", lambda e: e.step_actor(big, 2, noise=eps, std=std), True),
        ("policy_eval", lambda e: e.policy_eval(pol), False),
        ("actor_eval big on the device", lambda e: e.actor_eval(_on_device(big), features=_cuda(cot)[0]), False),
        ("step_policy", lambda e: e.step_policy(pol, 2), True),
        ("step_actor small", lambda e: e.step_actor(small, 1), True),
        ("actor_eval big again", lambda e: e.actor_eval(big), False),
    ]
    env = _make(E, N, Ng, M)
    for i, (name, call, steps) in enumerate(calls):
        fresh = _make(E, N, Ng, M)                          # the state comes from the stepping calls alone: replay those
        for _, earlier, stepped in calls[:i]:
            if stepped:
                earlier(fresh)
        got, want = results(call(env)), results(call(fresh))
        assert len(got) == len(want) and all(np.array_equal(p, q) for p, q in zip(got, want)), name
        assert _same(_state(env)[:2], _state(fresh)[:2]), name
        fresh.close()
    assert env.bad_count() == 0
    env.close()


# ---- 8. the contract ------------------------------------------------------------------------------------------------------------
def _spec(env, actor):
    from ocplasma_amd.env._arrays import Mem
    return actor.spec(Mem.of(env), env.num_envs)


def _rc_step(env, spec, nsteps=1, kind=0):
    return env._h.lib.pic_step_actor(env._h._h, ctypes.byref(spec), None, None, kind, nsteps, None, None, None, None)


def _rc_eval(env, spec, kind=0, features=None, x=None, v=None):
    p = [None if a is None else ctypes.c_void_p(a.__array_interface__["data"][0]) for a in (features, x, v)]
    return env._h.lib.pic_actor_eval(env._h._h, ctypes.byref(spec), *p, None, None, kind, None, None, None)


def _err(env):
    return env._h.lib.pic_last_error(env._h._h).decode()


def _tape_stats(env):
    s = env.tape_stats()
    return s if isinstance(s, dict) else {k: getattr(s, k) for k in dir(s) if not k.startswith("_")}


@pytest.mark.parametrize("pool_ln", [False, True])
def test_contract(pool_ln):
    from ocplasma_amd import _abi
    from ocplasma_amd._abi import PicError
    E, N, Ng, M, H = 2, 63, 32, 2, 5
    actor = _actor(H, 1, True, "relu", M, pool_ln, seed=1)
    env = _make(E, N, Ng, M)
    before, stats = _state(env), str(_tape_stats(env))
    feats, X = np.zeros((E, H)), np.zeros((E, N))

    def refused(code, reason, nsteps=1, kind=0, inner=None, **fields):
        spec, keep = _spec(env, actor)
        for k, v in fields.items():
            if k.startswith("width"):
                spec.width[int(k[5:])] = v
            else:
                setattr(spec, k, v)
        for k, v in (inner or {}).items():
            setattr((spec.pool_ln if pool_ln else spec.pool).contents, k, v)
        for rc in (_rc_step(env, spec, nsteps, kind), _rc_eval(env, spec, kind), _rc_eval(env, spec, kind, features=feats)):
            assert rc == code and reason in _err(env), (fields, inner, rc, _err(env))
            assert _same(_state(env), before) and str(_tape_stats(env)) == stats, fields

    spec, keep = _spec(env, actor)
    assert _rc_eval(env, spec) == 0 and _rc_eval(env, spec, features=feats) == 0 and _rc_step(env, spec, 0) == 0
    assert _same(_state(env), before)
    other = _abi.PicPoolSpec(H, 0, 0, 0, 1.0, keep[1].__array_interface__["data"][0])
    other_ln = _abi.PicPoolLnSpec(H, 0, 0, 0, 1.0, 1e-5, 0.0, keep[1].__array_interface__["data"][0])
    if pool_ln:
        refused(EINVAL, "exactly one of pool and pool_ln", pool=ctypes.pointer(other))
        refused(EINVAL, "exactly one of pool and pool_ln", pool_ln=None)
        refused(EINVAL, "eps must be finite and > 0", inner=dict(eps=0.0))
        refused(EINVAL, "period must be finite and >= 0", inner=dict(period=-1.0))
    else:
        refused(EINVAL, "exactly one of pool and pool_ln", pool_ln=ctypes.pointer(other_ln))
        refused(EINVAL, "exactly one of pool and pool_ln", pool=None)
    refused(EINVAL, "hidden must be 1..256", inner=dict(hidden=257), width0=257)
    refused(EINVAL, "activation must be", inner=dict(activation=2))
    refused(EINVAL, "per_env must be 0 or 1", inner=dict(per_env=2))
    refused(EINVAL, "bad params_mem_kind", inner=dict(params_mem_kind=2))
    refused(EINVAL, "params is NULL", inner=dict(params=None))
    refused(EINVAL, "v_scale is not finite", inner=dict(v_scale=float("inf")))
    refused(EINVAL, "n_layers", n_layers=0)
    refused(EINVAL, "n_layers", n_layers=7)
    refused(EINVAL, "every width", width1=257)
    refused(EINVAL, "every width", width2=0)
    refused(EINVAL, "width[0]", width0=H + 1)
    refused(EINVAL, "last width", width3=2 * M + 2)
    refused(EINVAL, "last width", n_layers=2)                           # the chain now ends at width[2] = 1
    refused(EINVAL, "layernorm", layernorm=2)
    refused(EINVAL, "squash", squash=-1)
    refused(EINVAL, "per_env must be 0 or 1", per_env=2)
    refused(EINVAL, "activation must be", activation=2)
    refused(EINVAL, "ln_eps", ln_eps=0.0)
    refused(EINVAL, "ln_eps", ln_eps=float("nan"))
    refused(EINVAL, "action_scale", action_scale=float("inf"))
    refused(EINVAL, "action_scale", action_shift=float("nan"))
    refused(EINVAL, "null params", params=None)
    refused(EINVAL, "mem_kind", kind=2)
    # the checks an actor shares with the MLP policy (csrc/host_head.h), in their own words ...
    last = f"the last width must be 2 max_mode of the actuator (pic_set_actuator) = {2 * M}"
    for reason, fields in (("bad mem_kind", dict(kind=2)), ("n_layers must be 1..6", dict(n_layers=7)),
                           ("every width must be 1..256", dict(width1=257)),
                           ("activation must be PIC_ACT_TANH or PIC_ACT_RELU", dict(activation=2)),
                           ("squash must be 0 or 1", dict(squash=2)), ("per_env must be 0 or 1", dict(per_env=2)),
                           ("null params", dict(params=None)), (last, dict(width3=2 * M + 2))):
        for nsteps in (1, 0):
            refused(EINVAL, ": " + reason, nsteps=nsteps, **fields)
    # ... and of two faults at once the one that is checked first, with steps and without
    for nsteps in (1, 0):
        refused(EINVAL, "bad mem_kind", nsteps=nsteps, kind=2, width1=257)
        refused(EINVAL, "bad mem_kind", nsteps=nsteps, kind=2, inner=dict(hidden=257))
        refused(EINVAL, "hidden must be 1..256", nsteps=nsteps, inner=dict(hidden=257), n_layers=7)
        refused(EINVAL, "n_layers must be 1..6", nsteps=nsteps, n_layers=7, width1=257)
        refused(EINVAL, "every width must be 1..256", nsteps=nsteps, width1=257, width0=H + 1)
        refused(EINVAL, "width[0] must be the pool's hidden", nsteps=nsteps, width0=H + 1, layernorm=2)
        refused(EINVAL, "layernorm must be 0 or 1", nsteps=nsteps, layernorm=2, activation=2)
        refused(EINVAL, "per_env must be 0 or 1", nsteps=nsteps, per_env=2, ln_eps=0.0)
        refused(EINVAL, "ln_eps must be finite and > 0", nsteps=nsteps, ln_eps=0.0, params=None)
        refused(EINVAL, "null params", nsteps=nsteps, params=None, width3=2 * M + 2)
    lib, hh = env._h.lib, env._h._h
    assert lib.pic_actor_eval(hh, None, None, None, None, None, None, 0, None, None, None) == EINVAL and "pic_actor_eval: null actor" in _err(env)
    assert lib.pic_step_actor(hh, None, None, None, 0, 1, None, None, None, None) == EINVAL and "pic_step_actor: null actor" in _err(env)
    assert _rc_step(env, spec, -1) == EINVAL and "nsteps" in _err(env)
    assert _rc_eval(env, spec, features=feats, x=X, v=X) == EINVAL and "features must not be given together" in _err(env)
    assert _rc_eval(env, spec, features=feats, v=X) == EINVAL and "features must not be given together" in _err(env)
    assert _rc_eval(env, spec, x=X) == EINVAL and "x and v must both be given or both be NULL" in _err(env)
    assert _rc_eval(env, spec, v=X) == EINVAL and "x and v must both be given or both be NULL" in _err(env)
    assert _same(_state(env), before) and str(_tape_stats(env)) == stats
    # PIC_ESTATE: a tape open (pic_step_actor alone: an evaluation changes nothing), before reset, without an actuator
    env.start_tape(4)
    open_stats = str(_tape_stats(env))
    assert _rc_step(env, spec) == ESTATE and "tape" in _err(env) and "torch policy" in _err(env)
    assert _rc_eval(env, spec) == 0 and str(_tape_stats(env)) == open_stats
    with pytest.raises(PicError, match="error -3: pic_step_actor: refused while a tape is open"):
        env.step_actor(actor, 1)
    env.stop_tape()
    assert _same(_state(env), before)
    fresh = _make(E, N, Ng, M, reset=False)
    assert _rc_step(fresh, spec) == ESTATE and "pic_reset" in _err(fresh)
    assert _rc_eval(fresh, spec) == ESTATE and "pic_reset" in _err(fresh)
    assert _rc_eval(fresh, spec, features=feats) == 0 and _rc_eval(fresh, spec, x=X, v=X) == 0      # (no stored particles are read)
    fresh.close()
    bare = _make(E, N, Ng, M, actuator=False)
    x0 = _state(bare)
    wrong, keep_wrong = _spec(env, actor)
    wrong.width[3] = 2 * M + 2                   # (a missing actuator is reported before a last width that would not fit one)
    for rc in (_rc_step(bare, spec), _rc_eval(bare, spec), _rc_eval(bare, spec, features=feats), _rc_step(bare, wrong),
               _rc_step(bare, wrong, 0), _rc_eval(bare, wrong), _rc_eval(bare, wrong, features=feats)):
        assert rc == ESTATE and ": call pic_set_actuator first" in _err(bare)
    assert _same(_state(bare), x0)
    bare.close()
    f32 = _make(E, N, Ng, M, dtype="float32")
    x0 = _state(f32)
    for rc in (_rc_step(f32, spec), _rc_step(f32, spec, 0), _rc_eval(f32, spec)):
        assert rc == EINVAL and "float64 particles with float64 positions" in _err(f32)
    assert _rc_eval(f32, spec, features=feats) == 0 and _rc_eval(f32, spec, x=X, v=X) == 0
    assert _same(_state(f32), x0)
    f32.close()
    # inside a staged step: refused where the stored particles are read, allowed on given features or particles
    staged = _make(E, N, Ng, M)
    staged._h.step_stage(1, np.zeros((E, Ng)))
    x0, st0 = _state(staged), str(_tape_stats(staged))
    assert _rc_eval(staged, spec) == ESTATE and "pic_actor_eval: a staged step is in progress" in _err(staged)
    for n in (1, 0):
        assert _rc_step(staged, spec, n) == ESTATE and "pic_step_actor: a staged step is in progress" in _err(staged)
    assert _rc_eval(staged, spec, features=feats) == 0 and _rc_eval(staged, spec, x=X, v=X) == 0
    assert _same(_state(staged), x0) and str(_tape_stats(staged)) == st0
    staged.close()
    # ... and after all the refusals the handle steps as one that saw none
    twin = _make(E, N, Ng, M)
    r, q = env.step_actor(actor, 2), twin.step_actor(actor, 2)
    assert np.array_equal(r.actions, q.actions) and _same(_state(env), _state(twin)) and env.bad_count() == 0
    env.close()
    twin.close()


# ---- 9. the torch twin --------------------------------------------------------------------------------------------------------------
def test_the_twin_follows_the_actor():
    """to_torch under rollout_policy(observe="state"): its first-step actions are step_actor's from the same state within test
    1's bound (torch's layers sum in another order); with_torch of perturbed parameters, and step_actor follows."""
    import torch
    from ocplasma_amd.env.grad import rollout_policy
    bound = 100 * ha.eval_floor()
    E, N, Ng, M = 2, 1025, 64, 2
    actor = _actor(5, 2, True, "relu", M, True, seed=4)
    unit = max(1.0, abs(actor.action_scale) + abs(actor.action_shift))
    for step in range(2):
        a, b = _make(E, N, Ng, M), _make(E, N, Ng, M)
        b.use_torch_stream()
        twin = actor.to_torch(b)
        acts = rollout_policy(b, twin, 3, observe="state")[3]
        r = a.step_actor(actor, 3)
        err = float(np.max(np.abs(_np(acts.detach()[0]) - r.actions[0]))) / unit
        print(f"twin, round {step}: first-step actions differ by {err:.3g} (bound {bound:.3g})")
        assert err <= bound
        if step == 0:
            acts.sum().backward()                            # the existing route gives every parameter a gradient
            assert all(p.grad is not None for p in twin.parameters())
            with torch.no_grad():
                for p in twin.parameters():
                    p.add_(0.05 * torch.randn(p.shape, dtype=p.dtype, generator=torch.Generator().manual_seed(1)).to(p.device))
            moved = actor.with_torch(twin)
            assert not np.array_equal(moved.params, actor.params) and not np.array_equal(moved.W, actor.W)
            actor = moved
        a.close()
        b.close()
