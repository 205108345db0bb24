"""The MLP policy on the device (pic_policy_eval, pic_step_policy): one evaluation against the NumPy restatement
of its arithmetic (tests/hp_mlp_policy.py), the caller's noise, whole rollouts against the host loop policy_eval -> step_actions
they replace (bit for bit, on both schedules, in host and in device memory), the linear special case against pic_step_feedback,
every place pic_step_actions runs, and the C contract."""
import ctypes

import numpy as np
import pytest

import hp_mlp_policy as hm
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = hm.M
EINVAL, ESTATE = -1, -3


@pytest.fixture(scope="module")
def bound():
    """100 x the largest difference between the float64 restatement and its longdouble twin over the tanh / squash cases of
    test_policy_eval_against_the_restatement (1.16e-15 -> 1.16e-13; profiles/policy_rollout.md): a quantity of the references
    alone.  The device's tanh and NumPy's may differ in the last bits."""
    return 100 * hm.floor(hm.tanh_cases())


def _policy(widths, activation, params, **kw):
    from ocplasma_amd.control.policy import MLPPolicy
    return MLPPolicy(widths, activation, params, widths[0] // 2, **kw)


def _make(E, N, Ng, M_=M, seed=1, dtype="float64", reset=True, actuator=True, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, dtype=dtype, **kw)
    if reset:
        xs, vs = zip(*[po.synthetic_two_stream(N, L, seed=seed + 7 * e) for e in range(E)])
        x0, v0 = np.stack(xs).astype(dtype), np.stack(vs).astype(dtype)
        x0[x0 >= L] = 0.0
        env.reset(x0, v0)
    if actuator:
        env.set_actuator(oc.E_field(L, Ng, M_))
    return env


def _state(env):
    return [np.asarray(a).copy() for a in (*env.particles(), *env.fields(), *env.energies())]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


# ---- 1. one evaluation against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("Mo", hm.OBS_MODES)
@pytest.mark.parametrize("Ng", [33, 250])
@pytest.mark.parametrize("E", hm.ENVS)
def test_policy_eval_against_the_restatement(bound, E, Ng, Mo):
    env = _make(E, 1000, Ng)
    worst = 0.0
    for widths in hm.stacks(Mo):
        # relu: no transcendental, so the float64 restatement gives the device's bits
        c = hm.eval_case(E, Mo, widths, "relu", False)
        pol = _policy(widths, "relu", c["params"])
        o, u, a = env.policy_eval(pol, obs=c["obs"])
        ur, ar = hm.forward(**c)
        assert np.array_equal(o, c["obs"]) and np.array_equal(u, ur) and np.array_equal(a, ar), widths
        # ... on the current field: the observation is pic_get_modes', the rest follows from it
        o, u, a = env.policy_eval(pol)
        ek = env.modes(Mo)
        assert np.array_equal(o, np.concatenate([ek.real, ek.imag], axis=1)), widths
        ur, _ = hm.forward(**{**c, "obs": o})
        assert np.array_equal(u, ur) and np.array_equal(a, u), widths
        # an observation scale, multiplied in before the first layer
        sc = np.linspace(0.5, 3.0, 2 * Mo)
        _, u, _ = env.policy_eval(_policy(widths, "relu", c["params"], obs_scale=sc), obs=c["obs"])
        assert np.array_equal(u, hm.forward(**c, obs_scale=sc)[0]), widths
        # tanh networks and squashed outputs: within 100 x the references' own difference
        for activation, squash in (("tanh", False), ("tanh", True), ("relu", True)):
            c = hm.eval_case(E, Mo, widths, activation, squash)
            pol = _policy(widths, activation, c["params"], squash=squash, action_scale=c["action_scale"])
            _, u, a = env.policy_eval(pol, obs=c["obs"])
            ur, ar = hm.forward(**c)
            err = max(np.max(np.abs(u - ur)), np.max(np.abs(a - ar)))
            worst = max(worst, err)
            print(f"policy_eval E={E} Ng={Ng} Mo={Mo} widths={widths} {activation} squash={squash}: err={err:.3e} bound={bound:.3e}")
            assert err <= bound, (widths, activation, squash, err, bound)
    record_measure(f"policy_eval_err.E{E}.Ng{Ng}.Mo{Mo}", worst)
    env.close()


def test_per_environment_parameters_use_their_own_row():
    E, Mo = 3, 5
    widths = hm.stacks(Mo)[1]
    c = hm.eval_case(E, Mo, widths, "relu", False, seed=3, per_env=True)
    assert not np.array_equal(c["params"][0], c["params"][1])
    env = _make(E, 1000, 33)
    _, u, a = env.policy_eval(_policy(widths, "relu", c["params"], per_env=True), obs=c["obs"])
    assert np.array_equal(u, hm.forward(**c)[0])
    one = _make(1, 1000, 33)
    for e in range(E):
        _, ue, ae = one.policy_eval(_policy(widths, "relu", c["params"][e]), obs=c["obs"][e:e + 1])
        assert np.array_equal(ue[0], u[e]) and np.array_equal(ae[0], a[e]), e
    # the same through stack(), and from device memory
    from ocplasma_amd.control.policy import MLPPolicy
    import torch
    st = MLPPolicy.stack([_policy(widths, "relu", c["params"][e]) for e in range(E)])
    _, u2, _ = env.policy_eval(st, obs=torch.as_tensor(c["obs"], device="cuda"))
    assert u2.is_cuda and np.array_equal(_np(u2), u)
    env.close()
    one.close()


# ---- 2. the caller's noise --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squash", [False, True])
def test_noise_is_the_callers(bound, squash):
    E, Mo = 3, 2
    widths = hm.stacks(Mo)[1]
    rng = np.random.default_rng(8)
    env = _make(E, 1000, 33)
    pol = _policy(widths, "tanh", hm.make_params(widths, 2), squash=squash, action_scale=1.25)
    eps, std = rng.normal(size=(E, 2 * M)), rng.uniform(0.1, 0.7, 2 * M)
    _, mean, a0 = env.policy_eval(pol)
    _, pre, act = env.policy_eval(pol, noise=eps, std=std)
    assert np.array_equal(pre, mean + std * eps)
    _, pre1, _ = env.policy_eval(pol, noise=eps)                       # std = None means 1
    assert np.array_equal(pre1, mean + eps)
    _, prez, az = env.policy_eval(pol, noise=np.zeros((E, 2 * M)), std=std)
    assert np.array_equal(prez, mean) and np.array_equal(az, a0)       # a zero eps gives the deterministic bits
    if squash:
        assert np.max(np.abs(act - 1.25 * np.tanh(pre))) <= bound
    else:
        assert np.array_equal(act, pre)
    env.close()


# ---- 3. a rollout in one call is the host loop ------------------------------------------------------------------------------
T3, E3, N3, NG3, MO3 = 6, 3, 2000, 64, 3
_LOOPS = {}


def _rollout_policy(per_env=False):
    widths = [2 * MO3, 16, 2 * M]
    return _policy(widths, "tanh", hm.make_params(widths, 5, (E3,) if per_env else ()), squash=True, action_scale=1.0,
                   obs_scale=np.full(2 * MO3, 8.0), per_env=per_env)


def _noise(T=T3, E=E3):
    rng = np.random.default_rng(9)
    return rng.normal(size=(T, E, 2 * M)), rng.uniform(0.05, 0.3, 2 * M)


def _host_loop(env, pol, T, eps=None, std=None):
    """T x (policy_eval on the device -> step_actions on the device pointer); the per-step records and the final state."""
    obs, pre, act, en = [], [], [], []
    for t in range(T):
        o, u, a = env.policy_eval(pol, noise=None if eps is None else eps[t], std=std, on_device=True)
        env.step_actions_torch(a)
        obs.append(_np(o)), pre.append(_np(u)), act.append(_np(a)), en.append(env.energies())
    en = np.stack([np.stack(e) for e in en])                           # [T, 3, E]
    return dict(obs=np.stack(obs), pre=np.stack(pre), actions=np.stack(act), KE=en[:, 0], PE=en[:, 1], PE_reward=en[:, 2],
                state=_state(env))


def _loop3(bpe):
    """The reference loop of a schedule, computed once and shared."""
    if bpe not in _LOOPS:
        env = _make(E3, N3, NG3, blocks_per_env=bpe)
        assert env._h.schedule() == ("resident" if bpe < 0 else "streaming")
        eps, std = _noise()
        _LOOPS[bpe] = _host_loop(env, _rollout_policy(), T3, eps, std)
        env.close()
    return _LOOPS[bpe]


def _assert_rollout(r, ref, sl=slice(None)):
    for k in ("obs", "pre", "actions", "KE", "PE", "PE_reward"):
        assert np.array_equal(_np(getattr(r, k)), ref[k][sl]), k


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("bpe", [-1, 4])
def test_step_policy_is_the_host_loop(bpe, memory):
    import torch
    ref = _loop3(bpe)
    eps, std = _noise()
    pol = _rollout_policy()
    if memory == "device":
        eps, std = torch.as_tensor(eps, device="cuda"), torch.as_tensor(std, device="cuda")
        pol = pol.with_params(torch.as_tensor(pol.params, device="cuda"))
    env = _make(E3, N3, NG3, blocks_per_env=bpe)
    bad0 = env.bad_count()
    r = env.step_policy(pol, T3, noise=eps, std=std)
    assert (memory == "device") == hasattr(r.actions, "is_cuda")
    _assert_rollout(r, ref)
    assert _same(_state(env), ref["state"])
    assert env.bad_count() == bad0 == 0
    env.close()
    # one call of 6 steps equals two calls of 3 steps (the second without the energies' record: the asynchronous form)
    env = _make(E3, N3, NG3, blocks_per_env=bpe)
    r1 = env.step_policy(pol, 3, noise=eps[:3], std=std)
    r2 = env.step_policy(pol, 3, noise=eps[3:], std=std, history=False)
    env.sync()
    _assert_rollout(r1, ref, slice(0, 3))
    assert r2.KE is None
    for k in ("obs", "pre", "actions"):
        assert np.array_equal(_np(getattr(r2, k)), ref[k][3:]), k
    assert _same(_state(env), ref["state"])
    env.close()


@pytest.mark.parametrize("bpe", [-1, 4])
def test_step_policy_per_environment_and_no_noise(bpe):
    pol = _rollout_policy(per_env=True)
    a, b = _make(E3, N3, NG3, blocks_per_env=bpe), _make(E3, N3, NG3, blocks_per_env=bpe)
    ref = _host_loop(b, pol, 3)
    r = a.step_policy(pol, 3)
    _assert_rollout(r, ref)
    assert _same(_state(a), ref["state"])
    a.close()
    b.close()


# ---- 4. the linear special case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpe", [-1, 4])
def test_linear_policy_is_step_feedback(bpe):
    E, N, Ng, T, M_ = 3, 2000, 64, 5, 3
    W = np.diag(np.concatenate([-np.ones(M_), np.ones(M_)]))
    from ocplasma_amd.control.policy import MLPPolicy
    pol = MLPPolicy.from_layers([(W, np.zeros(2 * M_))], "tanh", M_)
    a, b = _make(E, N, Ng, M_=M_, blocks_per_env=bpe), _make(E, N, Ng, M_=M_, blocks_per_env=bpe)
    r = a.step_policy(pol, T)
    f = b.step_feedback(T, actions=True, history=True)
    assert np.array_equal(r.actions, f["actions"])                     # by value: a signed zero may differ
    assert np.array_equal(r.pre, r.actions)
    for p, q in zip(a.particles(), b.particles()):
        assert np.array_equal(p, q)
    a.close()
    b.close()


# ---- 5. wherever pic_step_actions runs --------------------------------------------------------------------------------------
VARIANTS = {"float32": dict(dtype="float32"), "fixed32": dict(dtype="float32", position_dtype="fixed32"),
            "tsc": dict(interpol="TSC"), "verlet": dict(integrator="verlet"), "recorder": dict()}


@pytest.mark.parametrize("bpe", [-1, 4])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_step_policy_wherever_step_actions_runs(variant, bpe):
    T = 3
    pol = _rollout_policy()
    eps, std = _noise(T)
    a, b = (_make(E3, N3, NG3, blocks_per_env=bpe, **VARIANTS[variant]) for _ in range(2))
    if variant == "recorder":
        for env in (a, b):
            env.start_recording(stride=2, modes=4, x_bins=16)
    ref = _host_loop(b, pol, T, eps, std)
    r = a.step_policy(pol, T, noise=eps, std=std)
    _assert_rollout(r, ref)
    assert _same(_state(a), ref["state"])
    if variant == "recorder":
        ra, rb = a.recorded(), b.recorded()
        assert len(ra) == len(rb) == 1
        for k in ("steps", "KE", "PE", "PE_reward", "field_energy", "Ek", "x_hist"):
            assert np.array_equal(np.asarray(getattr(ra, k)), np.asarray(getattr(rb, k))), k
    a.close()
    b.close()


# ---- 6. the contract ----------------------------------------------------------------------------------------------------------
def _spec(env, pol):
    from ocplasma_amd.env._arrays import Mem
    return pol.spec(Mem.of(env), env.num_envs)


def _rc_step(env, spec, nsteps=1, kind=0):
    return env._h.lib.pic_step_policy(env._h._h, ctypes.byref(spec), None, None, kind, nsteps, None, None, None, None)


def _rc_eval(env, spec, kind=0):
    return env._h.lib.pic_policy_eval(env._h._h, ctypes.byref(spec), None, None, None, kind, None, None, None)


def _err(env):
    return env._h.lib.pic_last_error(env._h._h).decode()


def test_contract():
    Ng, Mo = 33, 2
    widths = [2 * Mo, 7, 2 * M]
    pol = _policy(widths, "tanh", hm.make_params(widths, 1))
    env = _make(2, 1000, Ng)
    before = _state(env)

    def refused(code, reason, nsteps=1, kind=0, **fields):
        spec, keep = _spec(env, pol)
        for k, v in fields.items():
            if k.startswith("width"):
                spec.width[int(k[5:])] = v
            else:
                setattr(spec, k, v)
        for rc in (_rc_step(env, spec, nsteps, kind), _rc_eval(env, spec, kind)):
            assert rc == code and reason in _err(env), (fields, rc, _err(env))
            assert _same(_state(env), before), fields

    spec, keep = _spec(env, pol)
    assert _rc_eval(env, spec) == 0 and _rc_step(env, spec, 0) == 0 and _same(_state(env), before)
    refused(EINVAL, "n_layers", n_layers=0)
    refused(EINVAL, "n_layers", n_layers=5)
    refused(EINVAL, "width", width1=257)
    refused(EINVAL, "width", width1=0)
    refused(EINVAL, "width[0]", width0=2 * Mo + 2)
    refused(EINVAL, "width[0]", obs_modes=Mo + 1)
    refused(EINVAL, "last width", width2=2 * M + 2)
    refused(EINVAL, "last width", n_layers=1)                          # the chain now ends at width[1] = 7
    refused(EINVAL, "obs_modes", obs_modes=Ng, width0=2 * Ng)
    refused(EINVAL, "obs_modes", obs_modes=65, width0=130)
    refused(EINVAL, "mem_kind", kind=2)
    refused(EINVAL, "activation", activation=2)
    refused(EINVAL, "squash", squash=2)
    refused(EINVAL, "params", params=None)
    # the checks a policy shares with the particle actor (csrc/host_head.h), in their own words ...
    last = f"the last width must be 2 max_mode of the actuator (pic_set_actuator) = {2 * M}"
    for reason, fields in (("bad mem_kind", dict(kind=2)), ("n_layers must be 1..4", dict(n_layers=5)),
                           ("every width must be 1..256", dict(width1=257)),
                           ("activation must be PIC_ACT_TANH or PIC_ACT_RELU", dict(activation=2)),
                           ("squash must be 0 or 1", dict(squash=2)), ("per_env must be 0 or 1", dict(per_env=2)),
                           ("null params", dict(params=None)), (last, dict(width2=2 * M + 2))):
        for nsteps in (1, 0):
            refused(EINVAL, ": " + reason, nsteps=nsteps, **fields)
    # ... and of two faults at once the one that is checked first, with steps and without
    for nsteps in (1, 0):
        refused(EINVAL, "bad mem_kind", nsteps=nsteps, kind=2, width1=257)
        refused(EINVAL, "n_layers must be 1..4", nsteps=nsteps, n_layers=5, width1=257)
        refused(EINVAL, "obs_modes must be 1..64", nsteps=nsteps, obs_modes=65, width1=257)
        refused(EINVAL, "every width must be 1..256", nsteps=nsteps, width1=257, width0=2 * Mo + 2)
        refused(EINVAL, "width[0] must be 2 obs_modes", nsteps=nsteps, width0=2 * Mo + 2, activation=2)
        refused(EINVAL, "per_env must be 0 or 1", nsteps=nsteps, per_env=2, params=None)
        refused(EINVAL, "null params", nsteps=nsteps, params=None, width2=2 * M + 2)
    lib, hh = env._h.lib, env._h._h
    assert lib.pic_policy_eval(hh, None, None, None, None, 0, None, None, None) == EINVAL and "pic_policy_eval: null policy" in _err(env)
    assert lib.pic_step_policy(hh, None, None, None, 0, 1, None, None, None, None) == EINVAL and "pic_step_policy: null policy" in _err(env)
    assert _rc_step(env, spec, -1) == EINVAL and "nsteps" in _err(env)
    # PIC_ESTATE: a tape open (pic_step_policy alone: an evaluation changes nothing), before reset, without an actuator
    env.start_tape(4)
    assert _rc_step(env, spec) == ESTATE and "tape" in _err(env)
    assert _rc_eval(env, spec) == 0
    env.stop_tape()
    assert _same(_state(env), before)
    from ocplasma_amd._abi import PicError
    env.start_tape(4)
    with pytest.raises(PicError, match="error -3: pic_step_policy: refused while a tape is open"):
        env.step_policy(pol, 1)
    env.stop_tape()
    fresh = _make(2, 1000, Ng, reset=False)
    assert _rc_step(fresh, spec) == ESTATE and "pic_reset" in _err(fresh)
    assert _rc_eval(fresh, spec) == ESTATE and "pic_reset" in _err(fresh)
    fresh.close()
    bare = _make(2, 1000, Ng, actuator=False)
    x0 = _state(bare)
    wrong, keep_wrong = _spec(env, pol)
    wrong.width[2] = 2 * M + 2                   # (a missing actuator is reported before a last width that would not fit one)
    for rc in (_rc_step(bare, spec), _rc_eval(bare, spec), _rc_step(bare, wrong), _rc_step(bare, wrong, 0), _rc_eval(bare, wrong)):
        assert rc == ESTATE and ": call pic_set_actuator first" in _err(bare)
    assert _same(_state(bare), x0)
    bare.close()
    # ... and after all the refusals the handle steps as one that saw none
    twin = _make(2, 1000, Ng)
    r, q = env.step_policy(pol, 2), twin.step_policy(pol, 2)
    assert np.array_equal(r.actions, q.actions) and _same(_state(env), _state(twin)) and env.bad_count() == 0
    with pytest.raises(ValueError):
        env.step_policy(_policy(widths, "tanh", hm.make_params(widths, 1, (3,)), per_env=True), 1)      # 3 rows, 2 environments
    env.close()
    twin.close()
