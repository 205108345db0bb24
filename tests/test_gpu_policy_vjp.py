"""Policy gradients on the device (pic_policy_vjp, pic_tape_step_policy, pic_tape_backward_policy): the VJP
kernel against the NumPy restatement of its arithmetic (tests/hp_mlp_policy_vjp.py), the taped rollout against the untaped one bit
for bit, the VJP inside the reverse walk against the restatement applied step by step, the linear special case against the gain
law, env.grad.rollout_mlp against the torch-twin route it replaces, bitwise invariance, a mixed tape, and the C contract."""
import ctypes

import numpy as np
import pytest

import hp_mlp_policy as hm
import hp_mlp_policy_vjp as hv
from conftest import record_measure, rel_err
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = hm.M
EINVAL, ESTATE, ENOMEM = -1, -3, -4
# test 5: 100 x the larger of the twin route's accuracy at the parent (4.4e-14, profiles/policy_grad.md) and the relative difference
# measured between the twin route and tests/hp_policy.py's autograd at this test's shapes: 5.3e-15 at Ng 33, 1.313e-13 at Ng 250
# (profiles/policy_grad_device.md); rollout_mlp itself differs from the twin route by 1.5e-15 at most
TWIN_VS_AUTOGRAD = 1.313e-13
TWIN_BOUND = 100 * max(4.4e-14, TWIN_VS_AUTOGRAD)


@pytest.fixture(scope="module")
def bound():
    """100 x the largest difference between the float64 restatement of the VJP and its longdouble twin over the tanh / squash
    cases of test_policy_vjp_against_the_restatement: a quantity of the references alone (DESIGN.md 7p records it)."""
    return 100 * hv.floor(hv.tanh_cases())


def _policy(widths, activation, params, **kw):
    from ocplasma_amd.control.policy import MLPPolicy
    return MLPPolicy(widths, activation, params, widths[0] // 2, **kw)


def _make(E, N, Ng, M_=M, seed=1, reset=True, actuator=True, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    if reset:
        xs, vs = zip(*[po.synthetic_two_stream(N, L, seed=seed + 7 * e) for e in range(E)])
        x0, v0 = np.stack(xs), np.stack(vs)
        x0[x0 >= L] = 0.0
        env.reset(x0, v0)
    if actuator:
        env.set_actuator(oc.E_field(L, Ng, M_))
    return env


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _state(env):
    return [np.asarray(a).copy() for a in (*env.particles(), *env.fields(), *env.energies())]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


# ---- 1. pic_policy_vjp against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("Mo", hm.OBS_MODES)
@pytest.mark.parametrize("Ng", [33, 250])
@pytest.mark.parametrize("E", hm.ENVS)
def test_policy_vjp_against_the_restatement(bound, E, Ng, Mo):
    env = _make(E, 1000, Ng)
    worst = 0.0
    for widths in hm.stacks(Mo):
        # relu without squash: no transcendental, so the float64 restatement gives the device's bits
        for per_env, scale in ((False, None), (True, None), (False, np.linspace(0.5, 3.0, 2 * Mo))):
            c = hv.vjp_case(E, Mo, widths, "relu", False, per_env=per_env, obs_scale=scale)
            pol = _policy(widths, "relu", c["params"], per_env=per_env, obs_scale=scale)
            gp, go, gu = env.policy_vjp(pol, c["obs"], c["cot"])                 # (pre may be left out without squash)
            ge, gor, gur = hv.vjp(**c)
            assert np.array_equal(gp, ge if per_env else hv.sum_envs(ge)), (widths, per_env)
            assert np.array_equal(go, gor) and np.array_equal(gu, gur), (widths, per_env)
        # tanh networks and squashed outputs: within 100 x the references' own difference
        for activation, squash in (("tanh", False), ("tanh", True), ("relu", True)):
            c = hv.vjp_case(E, Mo, widths, activation, squash)
            pol = _policy(widths, activation, c["params"], squash=squash, action_scale=c["action_scale"])
            gp, go, gu = env.policy_vjp(pol, c["obs"], c["cot"], pre=c["pre"])
            ge, gor, gur = hv.vjp(**c)
            err = max(np.max(np.abs(gp - hv.sum_envs(ge))), np.max(np.abs(go - gor)), np.max(np.abs(gu - gur)))
            worst = max(worst, err)
            print(f"policy_vjp E={E} Ng={Ng} Mo={Mo} widths={widths} {activation} squash={squash}: err={err:.3e} bound={bound:.3e}")
            assert err <= bound, (widths, activation, squash, err, bound)
    record_measure(f"policy_vjp_err.E{E}.Ng{Ng}.Mo{Mo}", worst)
    env.close()


def test_policy_vjp_relu_at_exactly_zero_and_from_device_memory():
    """A unit with zero weights and bias has the pre-activation 0 exactly: relu passes no gradient through it (d = 0 at y = 0)."""
    import torch
    E, Mo = 3, 5
    widths = hm.stacks(Mo)[1]
    c = hv.vjp_case(E, Mo, widths, "relu", False, seed=6)
    layers = [(W.copy(), b.copy()) for W, b in hm.layers_of(widths, c["params"])]
    layers[0][0][3, :] = 0.0
    layers[0][1][3] = 0.0
    c["params"] = np.concatenate([a.ravel() for pair in layers for a in pair])
    env = _make(E, 1000, 33)
    pol = _policy(widths, "relu", c["params"])
    gp, go, gu = env.policy_vjp(pol, c["obs"], c["cot"])
    ge, gor, gur = hv.vjp(**c)
    assert np.array_equal(gp, hv.sum_envs(ge)) and np.array_equal(go, gor) and np.array_equal(gu, gur)
    gW0 = pol.unpack_grad(gp)[0]
    assert not gW0[0][3].any() and gW0[1][3] == 0.0                  # nothing reaches the dead unit's row
    dev = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    gp2, go2, gu2 = env.policy_vjp(pol.with_params(dev(c["params"])), dev(c["obs"]), dev(c["cot"]))
    assert gp2.is_cuda and np.array_equal(_np(gp2), gp) and np.array_equal(_np(go2), go) and np.array_equal(_np(gu2), gu)
    env.close()


# ---- the rollouts the tests below share ---------------------------------------------------------------------------------------
T6, E3, N3 = 6, 3, 2000


def _rollout_policy(Mo, activation="tanh", squash=True, per_env=False, E=E3, seed=5, scaled=True):
    widths = hm.stacks(Mo)[1]                                          # [2 Mo, 37, 5, 2M]
    return _policy(widths, activation, hm.make_params(widths, seed, (E,) if per_env else ()), squash=squash,
                   action_scale=1.25 if squash else 1.0, obs_scale=np.full(2 * Mo, 8.0) if scaled else None, per_env=per_env)


def _noise(T=T6, E=E3):
    rng = np.random.default_rng(9)
    return rng.normal(size=(T, E, 2 * M)), rng.uniform(0.05, 0.3, 2 * M)


_UNTAPED = {}


def _untaped(bpe, Ng, Mo):
    """step_policy of T6 steps on a schedule, computed once and shared."""
    key = (bpe, Ng, Mo)
    if key not in _UNTAPED:
        env = _make(E3, N3, Ng, blocks_per_env=bpe)
        assert env._h.schedule() == ("resident" if bpe < 0 else "streaming")
        eps, std = _noise()
        r = env.step_policy(_rollout_policy(Mo), T6, noise=eps, std=std)
        _UNTAPED[key] = ({k: _np(getattr(r, k)) for k in r._fields}, _state(env))
        env.close()
    return _UNTAPED[key]


# ---- 2. taped forward == untaped -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("every", [1, 2, 0])
@pytest.mark.parametrize("bpe,Ng,Mo", [(-1, 33, 2), (4, 250, 5)])
def test_taped_rollout_has_the_untaped_bits(bpe, Ng, Mo, every, memory):
    import torch
    ref, state = _untaped(bpe, Ng, Mo)
    eps, std = _noise()
    pol = _rollout_policy(Mo)
    if memory == "device":
        eps, std = torch.as_tensor(eps, device="cuda"), torch.as_tensor(std, device="cuda")
        pol = pol.with_params(torch.as_tensor(pol.params, device="cuda"))
    env = _make(E3, N3, Ng, blocks_per_env=bpe)
    env.start_tape(T6, every)
    r1 = env.tape_step_policy(pol, 3, noise=eps[:3], std=std)
    r2 = env.tape_step_policy(pol, 3, noise=eps[3:], std=std)
    assert (memory == "device") == hasattr(r1.actions, "is_cuda")
    for k in ("obs", "pre", "actions", "KE", "PE", "PE_reward"):
        assert np.array_equal(_np(getattr(r1, k)), ref[k][:3]) and np.array_equal(_np(getattr(r2, k)), ref[k][3:]), k
    assert _same(_state(env), state)
    rng = np.random.default_rng(3)
    g = env.backward_policy(d_KE=rng.normal(size=(T6, E3)), d_PE_reward=rng.normal(size=(T6, E3)))
    st = env.tape_stats()
    assert st["steps"] == T6 and st["replay_mismatches"] == 0
    assert np.isfinite(g["params"]).all() and np.any(g["params"] != 0.0)
    env.stop_tape()
    env.close()


# ---- 3. the VJP inside the walk is the contract -------------------------------------------------------------------------------
def _replay_contract(pol, rec, g, per_env):
    """The restatement applied to backward_policy's own a-bar_t and the recorded o_t, u_t, step by step with t descending."""
    T = rec["obs"].shape[0]
    terms, g_obs, g_pre = [], np.zeros_like(rec["obs"]), np.zeros_like(rec["pre"])
    for t in range(T - 1, -1, -1):
        ge, g_obs[t], g_pre[t] = hv.vjp(pol.widths, pol.activation, np.asarray(pol.params), rec["obs"][t], g["actions"][t],
                                        pre=rec["pre"][t], squash=pol.squash, action_scale=pol.action_scale,
                                        obs_scale=pol.obs_scale)
        terms.append(ge)
    gE = hv.accumulate(terms)
    return (gE if per_env else hv.sum_envs(gE)), g_obs, g_pre


@pytest.mark.parametrize("activation,squash,per_env", [("relu", False, False), ("relu", False, True), ("tanh", True, False),
                                                       ("tanh", False, True)])
@pytest.mark.parametrize("bpe,Ng,Mo", [(-1, 33, 2), (4, 250, 5)])
def test_vjp_inside_the_walk_is_the_contract(bound, bpe, Ng, Mo, activation, squash, per_env):
    pol = _rollout_policy(Mo, activation, squash, per_env)
    eps, std = _noise()
    env = _make(E3, N3, Ng, blocks_per_env=bpe)
    env.start_tape(T6, 2)
    r = env.tape_step_policy(pol, T6, noise=eps, std=std)
    rng = np.random.default_rng(4)
    g = env.backward_policy(d_PE_reward=rng.normal(size=(T6, E3)), d_KE=rng.normal(size=(T6, E3)),
                            d_actions=0.1 * rng.normal(size=(T6, E3, 2 * M)), d_obs=0.1 * rng.normal(size=(T6, E3, 2 * Mo)))
    assert env.tape_stats()["replay_mismatches"] == 0
    gp, go, gu = _replay_contract(pol, dict(obs=_np(r.obs), pre=_np(r.pre)), g, per_env)
    if activation == "relu" and not squash:
        assert np.array_equal(g["params"], gp) and np.array_equal(g["obs"], go) and np.array_equal(g["pre"], gu)
    else:
        err = max(np.max(np.abs(g["params"] - gp)), np.max(np.abs(g["obs"] - go)), np.max(np.abs(g["pre"] - gu)))
        print(f"walk contract bpe={bpe} Ng={Ng} {activation} squash={squash} per_env={per_env}: err={err:.3e} bound={bound:.3e} "
              f"max|a-bar|={np.max(np.abs(g['actions'])):.3e}")
        record_measure(f"policy_walk_err.bpe{bpe}.{activation}.squash{int(squash)}", err)
        assert err <= bound, (err, bound)                              # the bound of test 1
    env.stop_tape()
    env.close()


# ---- 4. the linear special case --------------------------------------------------------------------------------------------------
_LINEAR = {}


def _linear_pair(bpe):
    """A one-layer policy W = G, b = 0 and the gain law G on a twin environment: both backwards, computed once per schedule."""
    if bpe not in _LINEAR:
        from ocplasma_amd.control.policy import MLPPolicy
        E, N, Ng, T = 3, 2000, 33, 5
        rng = np.random.default_rng(2)
        G = np.diag(np.concatenate([-np.ones(M), np.ones(M)])) + rng.uniform(-0.3, 0.3, (2 * M, 2 * M))
        pol = MLPPolicy.from_layers([(G, np.zeros(2 * M))], "tanh", M)
        hist = rng.normal(size=(T, 3, E))
        a, b = _make(E, N, Ng, blocks_per_env=bpe), _make(E, N, Ng, blocks_per_env=bpe)
        a.start_tape(T, 2)
        r = a.tape_step_policy(pol, T)
        g = a.backward_policy(d_KE=hist[:, 0], d_PE=hist[:, 1], d_PE_reward=hist[:, 2])
        b.start_tape(T, 2)
        f = b.step_feedback_gain(G, T, actions=True, modes=True)
        want = b._h.tape_backward_feedback(hist, None, None, None)
        for env in (a, b):
            env.stop_tape()
            env.close()
        _LINEAR[bpe] = (pol, T, r, f, g, want)
    return _LINEAR[bpe]


@pytest.mark.parametrize("bpe", [-1, 4])
def test_linear_policy_is_the_gain_law(bpe):
    pol, T, r, f, g, want = _linear_pair(bpe)
    assert np.array_equal(r.actions, f["actions"]) and np.array_equal(r.obs, f["modes"])
    # sum_t a-bar_t m_t^T on the host in the reverse pass's order, environments ascending
    terms = [g["actions"][t][:, :, None] * r.obs[t][:, None, :] for t in range(T - 1, -1, -1)]
    gW = hv.sum_envs(hv.accumulate(terms))
    assert np.array_equal(pol.unpack_grad(g["params"])[0][0], gW)
    print(f"linear policy vs gain law bpe={bpe}: rel diff g_x0 {rel_err(g['x0'], want['g_x0']):.3e}, "
          f"g_v0 {rel_err(g['v0'], want['g_v0']):.3e}")
    assert np.array_equal(g["x0"], want["g_x0"]) and np.array_equal(g["v0"], want["g_v0"])


@pytest.mark.parametrize("bpe", [-1, 4])
def test_linear_policy_reports_the_gain_laws_g_actions(bpe):
    """The gain law's reverse pass forms a-bar = B^T e-bar twice: law_adjoint_kernel sums it one wave per coefficient for the path
    into the plasma, and g_actions reports adjoint_actions_kernel's sum in ascending mesh order.  A policy step does the same:
    g_actions is the second sum, as every backward and walk reports it."""
    pol, T, r, f, g, want = _linear_pair(bpe)
    d = rel_err(g["actions"], want["g_actions"])
    print(f"linear policy vs gain law bpe={bpe}: rel diff g_actions {d:.3e}")
    record_measure(f"policy_linear_vs_law_g_actions.bpe{bpe}", d)
    assert np.array_equal(g["actions"], want["g_actions"])


# ---- 5. against the route it replaces ------------------------------------------------------------------------------------------
def _cost(ke, pe, per, acts, w):
    return (ke * w[0]).sum() + (pe * w[1]).sum() + (per * w[2]).sum() + 0.05 * (acts ** 2).sum()


def _twin_route(env, pol, T, eps, std, w, every, kl=None):
    """env.grad.rollout_policy under the to_torch() twin with the same noise: the flat parameter gradient."""
    import torch
    from ocplasma_amd.env import grad
    module = pol.to_torch().to("cuda")
    step = [0]

    def policy(o):
        t = step[0]
        step[0] += 1
        u = module[:-1](o * torch.as_tensor(pol.obs_scale, device="cuda")) + std * eps[t]
        return pol.action_scale * torch.tanh(u)

    out = grad.rollout_policy(env, policy, T, observe="modes", obs_modes=pol.obs_modes, checkpoint_every=every, kl=kl)
    J = _cost(out[0], out[1], out[2], out[3], w)
    if kl is not None:
        J = J + 0.3 * out[5].sum()
    J.backward()
    lin = [m for m in module if hasattr(m, "weight")]
    return pol.pack([(_np(m.weight.grad), _np(m.bias.grad)) for m in lin]), _np(std.grad)


def _mlp_route(env, pol, T, eps, std, w, every, kl=None):
    import torch
    from ocplasma_amd.env import grad
    params = torch.as_tensor(pol.params, device="cuda").clone().requires_grad_(True)
    out = grad.rollout_mlp(env, pol, params, T, noise=eps, std=std, checkpoint_every=every, kl=kl)
    J = _cost(out[0], out[1], out[2], out[3], w)
    if kl is not None:
        J = J + 0.3 * out[6].sum()
    J.backward()
    return _np(params.grad), _np(std.grad)


@pytest.mark.parametrize("every,kl", [(1, False), (0, False), (0, True)])
@pytest.mark.parametrize("bpe,Ng,Mo", [(-1, 33, 2), (4, 250, 5)])
def test_rollout_mlp_against_the_twin_route(bpe, Ng, Mo, every, kl):
    import torch
    pol = _rollout_policy(Mo)                                          # tanh [2 Mo, 37, 5, 2M] with squash
    eps_h, std_h = _noise()
    w = torch.as_tensor(np.random.default_rng(6).normal(size=(3, T6, E3)), device="cuda")
    spec = None
    if kl:
        v = np.linspace(-6.0, 6.0, 32)
        feq = np.tile(np.exp(-0.5 * (v / 1.5) ** 2) + 1e-3, (16, 1))
        spec = dict(feq=feq / feq.sum(), vmin=-6.0, vmax=6.0)
    got = {}
    for name, route in (("twin", _twin_route), ("mlp", _mlp_route)):
        env = _make(E3, N3, Ng, blocks_per_env=bpe)
        eps = torch.as_tensor(eps_h, device="cuda")
        std = torch.as_tensor(std_h, device="cuda").requires_grad_(True)
        got[name] = route(env, pol, T6, eps, std, w, every, spec)
        env.stop_tape()
        env.close()
    ep, es = rel_err(got["mlp"][0], got["twin"][0]), rel_err(got["mlp"][1], got["twin"][1])
    print(f"rollout_mlp vs twin bpe={bpe} Ng={Ng} every={every} kl={kl}: params {ep:.3e} std {es:.3e} bound {TWIN_BOUND:.3e}")
    record_measure(f"rollout_mlp_vs_twin.bpe{bpe}.every{every}.kl{int(kl)}", max(ep, es))
    assert max(ep, es) < TWIN_BOUND, (ep, es)


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------
def _grads(E, bpe, every, pol, eps, std, hist, seed0=1):
    env = _make(E, N3, 250, blocks_per_env=bpe, seed=seed0)
    env.start_tape(T6, every)
    env.tape_step_policy(pol, T6, noise=eps, std=std)
    g = env.backward_policy(d_KE=hist[:, 0], d_PE=hist[:, 1], d_PE_reward=hist[:, 2])
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    env.close()
    return g


def test_gradients_are_bitwise_invariant():
    Mo = 5
    pol = _rollout_policy(Mo)
    eps, std = _noise()
    hist = np.random.default_rng(12).normal(size=(T6, 3, E3))
    ref = None
    for bpe, every in ((-1, 0), (2, 1), (4, 2), (-1, 3), (4, 0), (2, 3)):
        g = _grads(E3, bpe, every, pol, eps, std, hist)
        if ref is None:
            ref = g
        for k in ("params", "x0", "v0", "pre", "obs", "actions"):
            assert np.array_equal(g[k], ref[k]), (bpe, every, k)


def test_per_environment_gradient_is_the_environments_own():
    Mo = 5
    pol = _rollout_policy(Mo, per_env=True)
    eps, std = _noise()
    hist = np.random.default_rng(13).normal(size=(T6, 3, E3))
    g3 = _grads(E3, 4, 2, pol, eps, std, hist)
    one = _rollout_policy(Mo).with_params(np.asarray(pol.params)[1])
    g1 = _grads(1, 4, 2, one, eps[:, 1:2], std, hist[:, :, 1:2], seed0=8)      # environment 1 of the batch: seed 1 + 7
    assert np.array_equal(g3["params"][1], g1["params"])
    assert np.array_equal(g3["x0"][1], g1["x0"][0]) and np.array_equal(g3["v0"][1], g1["v0"][0])


# ---- 7. a mixed tape -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpe", [-1, 4])
def test_mixed_tape_backward_is_the_walk(bpe):
    E, Ng, Mo, T = E3, 250, M, 6
    pol = _rollout_policy(Mo, "tanh", True)
    rng = np.random.default_rng(14)
    G = np.diag(np.concatenate([-np.ones(M), np.ones(M)])) + rng.uniform(-0.2, 0.2, (2 * M, 2 * M))
    acts = rng.uniform(-1, 1, (2, E, 2 * M))
    hist = rng.normal(size=(T, 3, E))
    env = _make(E, N3, Ng, blocks_per_env=bpe)
    env.start_tape(T, 2)
    env.step_actions_traj(acts)
    env.tape_step_policy(pol, 2)
    env.step_feedback_gain(G, 2)
    assert env.tape_stats()["steps"] == T
    g = env.backward_policy(d_KE=hist[:, 0], d_PE=hist[:, 1], d_PE_reward=hist[:, 2])
    w = env.walk(Mo)
    for t in range(T - 1, -1, -1):
        s, _, g_act = w.step(d_energies=hist[t])
        assert s == t
        if t in (2, 3):                                              # a policy step without a direct cotangent: a-bar = B^T e-bar
            assert np.array_equal(g_act, g["actions"][t]), t
    g_x0, g_v0 = w.end()
    assert np.array_equal(g_x0, g["x0"]) and np.array_equal(g_v0, g["v0"])
    assert np.array_equal(env.tape_policy_grad(), g["params"])
    assert not g["actions"][:2].any() and not g["actions"][4:].any() and not g["obs"][:2].any() and not g["pre"][4:].any()
    env.stop_tape()
    env.close()


# ---- 8. the contract -----------------------------------------------------------------------------------------------------------------
def _spec(env, pol):
    from ocplasma_amd.env._arrays import Mem
    return pol.spec(Mem.of(env), env.num_envs)


def _rc_tape_step(env, spec, nsteps=1, kind=0):
    return env._h.lib.pic_tape_step_policy(env._h._h, ctypes.byref(spec), None, None, kind, nsteps, None, None, None, None)


def _rc_vjp(env, spec, obs, pre, cot, kind=0):
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    return env._h.lib.pic_policy_vjp(env._h._h, ctypes.byref(spec), p(obs), p(pre), p(cot), kind, None, None, None)


def _err(env):
    return env._h.lib.pic_last_error(env._h._h).decode()


def test_contract():
    from ocplasma_amd._abi import PicError
    Ng, Mo, E = 33, 2, 2
    widths = [2 * Mo, 7, 2 * M]
    pol = _policy(widths, "tanh", hm.make_params(widths, 1), squash=True)
    obs, pre, cot = (np.random.default_rng(s).normal(size=(E, n)) for s, n in ((1, 2 * Mo), (2, 2 * M), (3, 2 * M)))
    env = _make(E, 1000, Ng)
    spec, keep = _spec(env, pol)
    # PIC_ESTATE: without a tape, before reset, without an actuator
    assert _rc_tape_step(env, spec) == ESTATE and "tape" in _err(env)
    fresh = _make(E, 1000, Ng, reset=False)
    assert _rc_tape_step(fresh, spec) == ESTATE
    assert _rc_vjp(fresh, spec, obs, pre, cot) == 0                    # the VJP touches no state and needs no reset
    fresh.close()
    bare = _make(E, 1000, Ng, actuator=False)
    bare.start_tape(4)
    assert _rc_tape_step(bare, spec) == ESTATE and "pic_set_actuator" in _err(bare)
    assert _rc_vjp(bare, spec, obs, pre, cot) == ESTATE and "pic_set_actuator" in _err(bare)
    bare.stop_tape()
    bare.close()
    # PIC_EINVAL with a reason, nothing enqueued, state and tape length untouched
    env.start_tape(4, budget_bytes=0)
    before = _state(env)

    def refused(code, reason, nsteps=1, kind=0, **fields):
        spec, keep = _spec(env, pol)
        for k, v in fields.items():
            if k.startswith("width"):
                spec.width[int(k[5:])] = v
            else:
                setattr(spec, k, v)
        steps = env.tape_stats()["steps"]
        for rc in (_rc_tape_step(env, spec, nsteps, kind), _rc_vjp(env, spec, obs, pre, cot, kind)):
            assert rc == code and reason in _err(env), (fields, rc, _err(env))
            assert _same(_state(env), before) and env.tape_stats()["steps"] == steps, fields

    refused(EINVAL, "n_layers", n_layers=0)
    refused(EINVAL, "n_layers", n_layers=5)
    refused(EINVAL, "width", width1=257)
    refused(EINVAL, "width", width1=0)
    refused(EINVAL, "width[0]", width0=2 * Mo + 2)
    refused(EINVAL, "width[0]", obs_modes=Mo + 1)
    refused(EINVAL, "last width", width2=2 * M + 2)
    refused(EINVAL, "last width", n_layers=1)
    refused(EINVAL, "obs_modes", obs_modes=Ng, width0=2 * Ng)
    refused(EINVAL, "obs_modes", obs_modes=65, width0=130)
    refused(EINVAL, "mem_kind", kind=2)
    refused(EINVAL, "activation", activation=2)
    refused(EINVAL, "squash", squash=2)
    refused(EINVAL, "params", params=None)
    assert _rc_tape_step(env, spec, -1) == EINVAL and "nsteps" in _err(env)
    assert _rc_vjp(env, spec, obs, None, cot) == EINVAL and "squash" in _err(env)      # pre NULL with squash
    assert _rc_vjp(env, spec, None, pre, cot) == EINVAL and _rc_vjp(env, spec, obs, pre, None) == EINVAL
    assert _rc_vjp(env, spec, obs, pre, cot) == 0 and _same(_state(env), before)       # allowed under a tape
    # a second policy call of another shape
    env.tape_step_policy(pol, 1)
    after1 = _state(env)
    for other in (_policy([2 * Mo, 8, 2 * M], "tanh", hm.make_params([2 * Mo, 8, 2 * M], 1), squash=True),
                  _policy(widths, "relu", hm.make_params(widths, 1), squash=True),
                  _policy(widths, "tanh", hm.make_params(widths, 1), squash=False),
                  _policy(widths, "tanh", hm.make_params(widths, 1, (E,)), squash=True, per_env=True)):
        s2, keep2 = _spec(env, other)
        assert _rc_tape_step(env, s2) == EINVAL and "same shape" in _err(env)
        assert env.tape_stats()["steps"] == 1 and _same(_state(env), after1)
    # tangents refuse a tape with policy steps; step_policy under a tape stays refused
    with pytest.raises(PicError, match="error -1: .*policy steps are not built in forward mode"):
        env.tangent(d_actions=np.zeros((1, E, 2 * M)))
    with pytest.raises(PicError, match="error -1: .*policy steps are not built in forward mode"):
        env.tangent_walk(K=1)
    with pytest.raises(PicError, match="error -3: pic_step_policy: refused while a tape is open"):
        env.step_policy(pol, 1)
    # PIC_ENOMEM beyond max_steps, before any step runs
    assert _rc_tape_step(env, spec, 4) == ENOMEM and "max_steps" in _err(env)
    assert env.tape_stats()["steps"] == 1 and _same(_state(env), after1)
    env.tape_step_policy(pol, 3)                                       # ... and the tape still takes what fits
    assert env.tape_stats()["steps"] == 4
    env.stop_tape()
    # PIC_ENOMEM beyond budget_bytes: a budget the bare tape just fits leaves no room for the policy's record
    env.start_tape(4)
    need = env.tape_stats()["bytes"]
    env.stop_tape()
    env.start_tape(4, budget_bytes=need)
    x0 = _state(env)
    assert _rc_tape_step(env, spec) == ENOMEM and "budget_bytes" in _err(env)
    assert env.tape_stats()["steps"] == 0 and env.tape_stats()["bytes"] == need and _same(_state(env), x0)
    with pytest.raises(PicError, match="error -3: pic_tape_backward_policy"):
        env._h.tape_backward_policy(0, *([0] * 11))                    # no policy steps on this tape
    with pytest.raises(PicError, match="no steps of tape_step_policy"):
        env.backward_policy()
    env.stop_tape()
    env.close()
