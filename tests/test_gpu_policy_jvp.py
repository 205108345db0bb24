"""Forward mode through MLP-policy rollouts on the device (pic_policy_jvp, pic_tape_tangent_policy): the JVP kernel
against the NumPy restatement of its arithmetic (tests/hp_mlp_policy_jvp.py), K directions against K single ones bit for bit,
tangent_policy against the torch-twin route it replaces, duality with backward_policy on the same tape, the linear special case
against the gain law's tangent, bitwise invariance, a mixed tape, env.grad.rollout_mlp under forward_ad, and the C contract."""
import ctypes

import numpy as np
import pytest

import hp_mlp_policy as hm
import hp_mlp_policy_jvp as hj
import hp_policy_jvp_routes as routes
from conftest import record_measure, rel_err
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = hm.M
EINVAL, ESTATE, ENOMEM = -1, -3, -4
# test 3: 100 x the largest relative difference between the route tangent_policy replaces (env.grad.rollout_policy_jvp under the
# to_torch() twin) and torch forward mode of tests/hp_policy.py at this test's shapes, measured on the MI355X by
# profiles/policy_jvp_device.py --accuracy: 5.7e-15 at Ng 33 (M_o 2), 4.194e-13 at Ng 250 (M_o 5), either checkpoint interval
# (profiles/policy_jvp_device.md).  Parent code against a CPU reference, never the code under test; the ceiling is 1e-9.
TWIN_VS_FORWARD_MODE = 4.194e-13
TWIN_BOUND = 100 * TWIN_VS_FORWARD_MODE
# tests 4, 5, 7, 8: 100 x the duality gap of the existing dual pair at this test's shapes, rollout_policy_jvp against
# rollout_policy's backward under the same twin: 4.3e-16 at Ng 33, 5.70e-15 at Ng 250 (the same script and file; 3.7e-14 in
# DESIGN.md 7n at that section's own shapes)
TWIN_DUALITY_GAP = 5.70e-15
DUALITY_BOUND = 100 * TWIN_DUALITY_GAP


@pytest.fixture(scope="module")
def bound():
    """100 x the largest difference between the float64 restatement of the JVP and its longdouble twin over the tanh / squash
    cases of test_policy_jvp_against_the_restatement: a quantity of the references alone (DESIGN.md 7q records it)."""
    return 100 * hj.floor(hj.tanh_cases())


def _policy(widths, activation, params, **kw):
    from ocplasma_amd.control.policy import MLPPolicy
    return MLPPolicy(widths, activation, params, widths[0] // 2, **kw)


def _start(E, N, seed=1):
    xs, vs = zip(*[po.synthetic_two_stream(N, L, seed=seed + 7 * e) for e in range(E)])
    x0, v0 = np.stack(xs), np.stack(vs)
    x0[x0 >= L] = 0.0
    return x0, v0


def _make(E, N, Ng, seed=1, reset=True, actuator=True, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    if reset:
        env.reset(*_start(E, N, seed))
    if actuator:
        env.set_actuator(oc.E_field(L, Ng, M))
    return env


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _state(env):
    return [np.asarray(a).copy() for a in (*env.particles(), *env.fields(), *env.energies())]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _stack(cases, key):
    return None if cases[0][key] is None else np.stack([c[key] for c in cases])


KEYS = ("dKE", "dPE", "dPE_reward", "d_obs", "d_pre", "d_actions", "d_x", "d_v")


# ---- 1. pic_policy_jvp against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("Mo", hm.OBS_MODES)
@pytest.mark.parametrize("Ng", [33, 250])
@pytest.mark.parametrize("E", hm.ENVS)
def test_policy_jvp_against_the_restatement(bound, E, Ng, Mo):
    import torch
    env = _make(E, 1000, Ng)
    worst = 0.0
    dev = lambda a: None if a is None else torch.as_tensor(a, device="cuda")  # noqa: E731
    for widths in hm.stacks(Mo):
        # relu without squash: no transcendental, so the float64 restatement gives the device's bits
        for per_env, scale in ((False, None), (True, None), (False, np.linspace(0.5, 3.0, 2 * Mo))):
            for K in (1, 3, 8):
                cs = [hj.jvp_case(E, Mo, widths, "relu", False, seed=s, per_env=per_env, obs_scale=scale) for s in range(K)]
                for c in cs[1:]:                                         # one evaluation, K directions
                    c.update({k: cs[0][k] for k in ("params", "obs", "pre")})
                pol = _policy(widths, "relu", cs[0]["params"], per_env=per_env, obs_scale=scale)
                want = [hj.jvp(**c) for c in cs]
                du, da = env.policy_jvp(pol, cs[0]["obs"], d_params=_stack(cs, "d_params"), d_obs=_stack(cs, "d_obs"),
                                        d_pre=_stack(cs, "d_pre"))       # (pre may be left out without squash)
                assert du.shape == (K, E, 2 * M)
                for k in range(K):
                    assert np.array_equal(du[k], want[k][0]) and np.array_equal(da[k], want[k][1]), (widths, per_env, K, k)
                if K == 3:                                               # device memory: the same bits
                    du2, da2 = env.policy_jvp(pol.with_params(dev(cs[0]["params"])), dev(cs[0]["obs"]),
                                              d_params=dev(_stack(cs, "d_params")), d_obs=dev(_stack(cs, "d_obs")),
                                              d_pre=dev(_stack(cs, "d_pre")))
                    assert du2.is_cuda and np.array_equal(_np(du2), du) and np.array_equal(_np(da2), da)
        # tanh networks and squashed outputs: within 100 x the references' own difference
        for activation, squash in (("tanh", False), ("tanh", True), ("relu", True)):
            c = hj.jvp_case(E, Mo, widths, activation, squash)
            pol = _policy(widths, activation, c["params"], squash=squash, action_scale=c["action_scale"])
            du, da = env.policy_jvp(pol, c["obs"], pre=c["pre"], d_params=c["d_params"], d_obs=c["d_obs"], d_pre=c["d_pre"])
            assert du.shape == (E, 2 * M)                                # (no leading axis without one on the inputs)
            ur, ar = hj.jvp(**c)
            err = max(np.max(np.abs(du - ur)), np.max(np.abs(da - ar)))
            worst = max(worst, err)
            print(f"policy_jvp E={E} Ng={Ng} Mo={Mo} widths={widths} {activation} squash={squash}: err={err:.3e} bound={bound:.3e}")
            assert err <= bound, (widths, activation, squash, err, bound)
    record_measure(f"policy_jvp_err.E{E}.Ng{Ng}.Mo{Mo}", worst)
    env.close()


def test_policy_jvp_relu_at_exactly_zero_and_missing_tangents():
    """A unit with zero weights and bias has the pre-activation 0 exactly: relu passes no tangent through it (d = 0 at y = 0),
    whatever the tangent of its own weights.  A tangent left out is a tangent of zeros."""
    E, Mo = 3, 5
    widths = hm.stacks(Mo)[1]
    c = hj.jvp_case(E, Mo, widths, "relu", False, seed=6)
    layers = [(W.copy(), b.copy()) for W, b in hm.layers_of(widths, c["params"])]
    layers[0][0][3, :] = 0.0
    layers[0][1][3] = 0.0
    c["params"] = np.concatenate([a.ravel() for pair in layers for a in pair])
    env = _make(E, 1000, 33)
    pol = _policy(widths, "relu", c["params"])
    du, da = env.policy_jvp(pol, c["obs"], d_params=c["d_params"], d_obs=c["d_obs"], d_pre=c["d_pre"])
    ur, ar = hj.jvp(**c)
    assert np.array_equal(du, ur) and np.array_equal(da, ar)
    only = np.zeros_like(c["d_params"])
    only[3 * widths[0]:4 * widths[0]] = 1.0                              # dW_0[3][:] alone: it ends at the dead unit
    du, da = env.policy_jvp(pol, c["obs"], d_params=only)
    assert not du.any() and not da.any()
    for drop in ("d_params", "d_obs", "d_pre"):
        kw = {k: c[k] for k in ("d_params", "d_obs", "d_pre") if k != drop}
        du, da = env.policy_jvp(pol, c["obs"], **kw)
        ur, ar = hj.jvp(**{**c, drop: None})
        assert np.array_equal(du, ur) and np.array_equal(da, ar), drop
    env.close()


# ---- the rollouts the tests below share ---------------------------------------------------------------------------------------
T6, E3, N3 = 6, 3, 1000


def _rollout_policy(Mo, activation="tanh", squash=True, per_env=False, E=E3, seed=5, scaled=True):
    widths = hm.stacks(Mo)[1]                                          # [2 Mo, 37, 5, 2M]
    return _policy(widths, activation, hm.make_params(widths, seed, (E,) if per_env else ()), squash=squash,
                   action_scale=1.25 if squash else 1.0, obs_scale=np.full(2 * Mo, 8.0) if scaled else None, per_env=per_env)


def _noise(T=T6, E=E3):
    rng = np.random.default_rng(9)
    return rng.normal(size=(T, E, 2 * M)), rng.uniform(0.05, 0.3, 2 * M)


def _directions(pol, K, E=E3, N=N3, T=T6, seed=21, actions=False):
    """K random directions: parameters, std, a d_pre injection, x_0, v_0 (and a d_actions injection)."""
    rng = np.random.default_rng(seed)
    d = dict(d_params=rng.normal(size=(K,) + np.shape(pol.params)), d_std=rng.normal(size=(K, 2 * M)),
             d_pre=rng.normal(size=(K, T, E, 2 * M)), d_x0=rng.normal(size=(K, E, N)), d_v0=rng.normal(size=(K, E, N)))
    if actions:
        d["d_actions"] = rng.normal(size=(K, T, E, 2 * M))
    return d


def _taped(E, N, Ng, pol, eps, std, every, bpe, seed=1):
    """A fresh environment with T6 policy steps taped as 3 + 3."""
    env = _make(E, N, Ng, blocks_per_env=bpe, seed=seed)
    env.start_tape(T6, every)
    env.tape_step_policy(pol, 3, noise=eps[:3], std=std)
    env.tape_step_policy(pol, 3, noise=eps[3:], std=std)
    return env


# ---- 2. K directions are K single directions -----------------------------------------------------------------------------------
def test_k_directions_are_k_single_directions_bit_for_bit():
    E, Mo, K = 3, 5, 8
    widths = hm.stacks(Mo)[2]
    cs = [hj.jvp_case(E, Mo, widths, "tanh", True, seed=s) for s in range(K)]
    env = _make(E, 1000, 33)
    pol = _policy(widths, "tanh", cs[0]["params"], squash=True, action_scale=1.25)
    du, da = env.policy_jvp(pol, cs[0]["obs"], pre=cs[0]["pre"], d_params=_stack(cs, "d_params"), d_obs=_stack(cs, "d_obs"),
                            d_pre=_stack(cs, "d_pre"))
    for k, c in enumerate(cs):
        u1, a1 = env.policy_jvp(pol, cs[0]["obs"], pre=cs[0]["pre"], d_params=c["d_params"], d_obs=c["d_obs"], d_pre=c["d_pre"])
        assert np.array_equal(u1, du[k]) and np.array_equal(a1, da[k]), k
    env.close()
    pol = _rollout_policy(Mo)
    eps, std = _noise()
    env = _taped(E3, N3, 250, pol, eps, std, 2, 4)
    d = _directions(pol, 3, actions=True)
    d["noise"] = eps
    all3 = env.tangent_policy(**d, fields=True)
    for k in range(3):
        one = env.tangent_policy(**{n: (a if n == "noise" else a[k]) for n, a in d.items()}, fields=True)
        for key in KEYS + ("d_E_mesh",):
            assert np.array_equal(one[key], all3[key][k]), (k, key)
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    env.close()


# ---- 3. against the route it replaces ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 0])
@pytest.mark.parametrize("bpe,Ng,Mo", [(-1, 33, 2), (4, 250, 5)])
def test_tangent_policy_against_the_twin_route(bpe, Ng, Mo, every):
    import torch
    K = 2
    pol = _rollout_policy(Mo)                                          # tanh [2 Mo, 37, 5, 2M] with squash
    eps, std = _noise()
    d = _directions(pol, K)
    del d["d_pre"]
    env = _make(E3, N3, Ng, blocks_per_env=bpe)
    assert env._h.schedule() == ("resident" if bpe < 0 else "streaming")
    dx, dv = (torch.as_tensor(d[k], device="cuda") for k in ("d_x0", "d_v0"))
    want = routes.twin_route(env, routes.Twin(pol, eps, std), d["d_params"], d["d_std"], T6, dx, dv, checkpoint_every=every)
    env.stop_tape()
    env.close()
    env = _taped(E3, N3, Ng, pol, eps, std, every, bpe)
    got = env.tangent_policy(noise=eps, **d)
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    env.close()
    errs = {k: rel_err(got[k], want[k]) for k in ("dKE", "dPE", "dPE_reward", "d_actions", "d_x", "d_v")}
    print(f"tangent_policy vs twin bpe={bpe} Ng={Ng} every={every}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) +
          f" bound {TWIN_BOUND:.3e}")
    record_measure(f"tangent_policy_vs_twin.bpe{bpe}.every{every}", max(errs.values()))
    assert TWIN_BOUND <= 1e-9
    assert max(errs.values()) < TWIN_BOUND, errs


# ---- 4. duality with backward_policy on the same tape --------------------------------------------------------------------------
def _duality_gap(env, d, T, rng, E=E3, N=N3):
    """|<c, J d> - <J^T c, d>| relative to the larger inner product, over the whole batch (the parameters' term of a shared policy
    is a sum over environments), for one direction d without a leading axis on a tape of policy steps alone."""
    cot = {k: rng.normal(size=(T, E)) for k in ("KE", "PE", "PE_reward")}
    ca, cx, cv = rng.normal(size=(T, E, 2 * M)), rng.normal(size=(E, N)), rng.normal(size=(E, N))
    out = env.tangent_policy(**d)
    g = env.backward_policy(d_KE=cot["KE"], d_PE=cot["PE"], d_PE_reward=cot["PE_reward"], d_x=cx, d_v=cv, d_actions=ca)
    assert env.tape_stats()["replay_mismatches"] == 0
    lhs = float(sum((out["d" + k] * cot[k]).sum() for k in cot) + (out["d_actions"] * ca).sum()
                + (out["d_x"] * cx).sum() + (out["d_v"] * cv).sum())
    rhs = 0.0
    if "d_params" in d:
        rhs += float((g["params"] * d["d_params"]).sum())
    if "d_pre" in d:
        rhs += float((g["pre"] * d["d_pre"]).sum())
    if "d_actions" in d:
        rhs += float((g["actions"] * d["d_actions"]).sum())
    rhs += float((g["x0"] * d["d_x0"]).sum() + (g["v0"] * d["d_v0"]).sum())
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs)), out


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("bpe,Ng,Mo,every", [(-1, 33, 2, 2), (4, 250, 5, 0)])
def test_tangent_policy_is_dual_to_backward_policy(bpe, Ng, Mo, every, per_env):
    pol = _rollout_policy(Mo, per_env=per_env)
    eps, std = _noise()
    env = _taped(E3, N3, Ng, pol, eps, std, every, bpe)
    d = {k: a[0] for k, a in _directions(pol, 1, seed=22).items() if k != "d_std"}
    gap, _ = _duality_gap(env, d, T6, np.random.default_rng(23))
    env.stop_tape()
    env.close()
    print(f"tangent_policy / backward_policy duality bpe={bpe} Ng={Ng} per_env={per_env}: gap {gap:.3e} bound {DUALITY_BOUND:.3e}")
    record_measure(f"tangent_policy_duality.bpe{bpe}.per_env{int(per_env)}", gap)
    assert gap < DUALITY_BOUND, gap


# ---- 5. the linear special case --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpe", [-1, 4])
def test_linear_policy_is_the_gain_laws_tangent(bpe):
    """One layer W = G, b = 0 without squash: d_params = (dG, 0) is the gain's tangent.  The two sides sum G dm + dG m in
    different orders, so the agreement is to rounding, not bits."""
    from ocplasma_amd.control.policy import MLPPolicy
    E, N, Ng, T, K = 3, 1000, 33, 5, 2
    rng = np.random.default_rng(2)
    G = np.diag(np.concatenate([-np.ones(M), np.ones(M)])) + rng.uniform(-0.3, 0.3, (2 * M, 2 * M))
    dG = rng.normal(size=(K, 2 * M, 2 * M))
    dx, dv = rng.normal(size=(K, E, N)), rng.normal(size=(K, E, N))
    pol = MLPPolicy.from_layers([(G, np.zeros(2 * M))], "tanh", M)
    a, b = _make(E, N, Ng, blocks_per_env=bpe), _make(E, N, Ng, blocks_per_env=bpe)
    a.start_tape(T, 2)
    a.tape_step_policy(pol, T)
    got = a.tangent_policy(d_params=np.stack([pol.pack_tangent([(dG[k], None)]) for k in range(K)]), d_x0=dx, d_v0=dv)
    b.start_tape(T, 2)
    b.step_feedback_gain(G, T)
    want = b.tangent_feedback(d_gain=np.broadcast_to(dG[:, None], (K, E, 2 * M, 2 * M)).copy(), d_x0=dx, d_v0=dv)
    for env in (a, b):
        assert env.tape_stats()["replay_mismatches"] == 0
        env.stop_tape()
        env.close()
    errs = {k: rel_err(got[g], want[k]) for g, k in (("dKE", "KE"), ("dPE", "PE"), ("dPE_reward", "PE_reward"), ("d_actions", "actions"),
                                                     ("d_obs", "modes"), ("d_x", "x"), ("d_v", "v"))}
    print(f"linear policy vs gain law's tangent bpe={bpe}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    record_measure(f"tangent_policy_linear_vs_law.bpe{bpe}", max(errs.values()))
    assert max(errs.values()) < DUALITY_BOUND, errs


# ---- 6. invariance -----------------------------------------------------------------------------------------------------------------
def test_tangents_are_bitwise_invariant():
    import torch
    Mo, K = 5, 2
    pol = _rollout_policy(Mo)
    eps, std = _noise()
    d = _directions(pol, K, actions=True)
    ref = None
    for bpe, every in ((-1, 0), (2, 1), (4, 2), (-1, 3), (4, 0), (2, 3)):
        env = _taped(E3, N3, 250, pol, eps, std, every, bpe)
        outs = [env.tangent_policy(noise=eps, **d)]
        if (bpe, every) == (4, 2):                                     # host against device memory
            outs.append(env.tangent_policy(noise=torch.as_tensor(eps, device="cuda"),
                                           **{k: torch.as_tensor(a, device="cuda") for k, a in d.items()}))
            assert outs[1]["d_x"].is_cuda
        assert env.tape_stats()["replay_mismatches"] == 0
        env.stop_tape()
        env.close()
        ref = outs[0] if ref is None else ref
        for out in outs:
            for k in KEYS:
                assert np.array_equal(_np(out[k]), ref[k]), (bpe, every, k)


def test_per_environment_tangent_is_the_environments_own():
    Mo, K = 5, 2
    pol = _rollout_policy(Mo, per_env=True)
    eps, std = _noise()
    d = _directions(pol, K, actions=True)
    env = _taped(E3, N3, 250, pol, eps, std, 2, 4)
    g3 = env.tangent_policy(noise=eps, **d)
    env.stop_tape()
    env.close()
    one = _rollout_policy(Mo).with_params(np.asarray(pol.params)[1])
    env = _taped(1, N3, 250, one, eps[:, 1:2], std, 2, 4, seed=8)     # environment 1 of the batch: seed 1 + 7
    d1 = {k: (a[:, 1] if k == "d_params" else a if k == "d_std" else a[..., 1:2, :]) for k, a in d.items()}
    g1 = env.tangent_policy(noise=eps[:, 1:2], **d1)
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    env.close()
    for k in ("dKE", "dPE", "dPE_reward"):
        assert np.array_equal(g3[k][:, :, 1], g1[k][:, :, 0]), k
    for k in ("d_obs", "d_pre", "d_actions"):
        assert np.array_equal(g3[k][:, :, 1], g1[k][:, :, 0]), k
    assert np.array_equal(g3["d_x"][:, 1], g1["d_x"][:, 0]) and np.array_equal(g3["d_v"][:, 1], g1["d_v"][:, 0])


# ---- 7. a mixed tape -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpe", [-1, 4])
def test_mixed_tape_is_finite_and_dual_to_backward_policy(bpe):
    E, Ng, Mo, T = E3, 250, M, 6
    pol = _rollout_policy(Mo, "tanh", True)
    rng = np.random.default_rng(14)
    G = np.diag(np.concatenate([-np.ones(M), np.ones(M)])) + rng.uniform(-0.2, 0.2, (2 * M, 2 * M))
    env = _make(E, N3, Ng, blocks_per_env=bpe)
    env.start_tape(T, 2)
    env.step_actions_traj(rng.uniform(-1, 1, (2, E, 2 * M)))
    env.tape_step_policy(pol, 2)
    env.step_feedback_gain(G, 2)
    assert env.tape_stats()["steps"] == T
    da = np.zeros((T, E, 2 * M))
    da[:2] = rng.normal(size=(2, E, 2 * M))                            # only the actions steps are driven
    dx = rng.normal(size=(E, N3))
    cot = {k: rng.normal(size=(T, E)) for k in ("KE", "PE", "PE_reward")}
    cx, cv = rng.normal(size=(E, N3)), rng.normal(size=(E, N3))
    out = env.tangent_policy(d_actions=da, d_x0=dx)
    kw = dict(d_KE=cot["KE"], d_PE=cot["PE"], d_PE_reward=cot["PE_reward"], d_x=cx, d_v=cv)
    g = env.backward_policy(**kw)
    ab = env.backward(**kw)["actions"]             # a-bar of every step (backward_policy reports the policy steps' alone)
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    env.close()
    for k in KEYS:
        assert np.isfinite(out[k]).all(), k
    assert np.array_equal(out["d_actions"][:2], da[:2])                # an actions step takes d_actions as its whole tangent
    assert not out["d_pre"][:2].any() and not out["d_pre"][4:].any() and out["d_pre"][2:4].any()
    assert np.array_equal(ab[2:4], g["actions"][2:4])
    lhs = float(sum((out["d" + k] * cot[k]).sum() for k in cot) + (out["d_x"] * cx).sum() + (out["d_v"] * cv).sum())
    rhs = float((ab[:2] * da[:2]).sum() + (g["x0"] * dx).sum())
    gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"mixed tape duality bpe={bpe}: gap {gap:.3e} bound {DUALITY_BOUND:.3e}")
    record_measure(f"tangent_policy_mixed_duality.bpe{bpe}", gap)
    assert gap < DUALITY_BOUND, gap


# ---- 8. rollout_mlp under forward_ad ---------------------------------------------------------------------------------------------
def test_rollout_mlp_under_forward_ad():
    import torch
    import torch.autograd.forward_ad as fwAD
    from ocplasma_amd.env import grad
    Mo, Ng = 5, 250
    pol = _rollout_policy(Mo)
    eps_h, std_h = _noise()
    d = _directions(pol, 1, seed=31)
    t = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    eps, std, params = t(eps_h), t(std_h), t(np.asarray(pol.params))
    env = _make(E3, N3, Ng, blocks_per_env=4)
    with fwAD.dual_level():
        outs = grad.rollout_mlp(env, pol, fwAD.make_dual(params, t(d["d_params"][0])), T6, noise=eps,
                                std=fwAD.make_dual(std, t(d["d_std"][0])), checkpoint_every=2)
        tans = [fwAD.unpack_dual(o).tangent for o in outs]
        want = env.tangent_policy(d_params=t(d["d_params"][0]), d_std=t(d["d_std"][0]), noise=eps)
    for got, k in zip(tans, ("dKE", "dPE", "dPE_reward", "d_actions", "d_pre", "d_obs")):
        assert torch.equal(got, want[k]), k
    env.stop_tape()
    # ... and that JVP is dual to rollout_mlp's own backward
    p = params.clone().requires_grad_(True)
    s = std.clone().requires_grad_(True)
    env.reset(*_start(E3, N3, 1))
    outs = grad.rollout_mlp(env, pol, p, T6, noise=eps, std=s, checkpoint_every=2)
    rng = np.random.default_rng(32)
    w = [t(rng.normal(size=tuple(o.shape))) for o in outs[:4]]
    sum((o * c).sum() for o, c in zip(outs[:4], w)).backward()
    lhs = float(sum((a * c).sum() for a, c in zip(tans[:4], w)))
    rhs = float((p.grad * t(d["d_params"][0])).sum() + (s.grad * t(d["d_std"][0])).sum())
    gap = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    print(f"rollout_mlp forward_ad / backward duality: gap {gap:.3e} bound {DUALITY_BOUND:.3e}")
    record_measure("rollout_mlp_forward_ad_duality", gap)
    assert gap < DUALITY_BOUND, gap
    # with kl= the JVP is refused, as rollout_feedback's is
    v = np.linspace(-6.0, 6.0, 32)
    feq = np.tile(np.exp(-0.5 * (v / 1.5) ** 2) + 1e-3, (16, 1))
    env.stop_tape()
    env.reset(*_start(E3, N3, 1))
    with fwAD.dual_level(), pytest.raises(NotImplementedError, match="KL"):
        grad.rollout_mlp(env, pol, fwAD.make_dual(params, t(d["d_params"][0])), T6, noise=eps, std=std,
                         kl=dict(feq=feq / feq.sum(), vmin=-6.0, vmax=6.0))
    env.stop_tape()
    env.close()


# ---- 9. the contract -----------------------------------------------------------------------------------------------------------------
def _spec(env, pol):
    from ocplasma_amd.env._arrays import Mem
    return pol.spec(Mem.of(env), env.num_envs)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _rc_jvp(env, spec, obs, pre, K=1, kind=0, out=None):
    return env._h.lib.pic_policy_jvp(env._h._h, ctypes.byref(spec), _p(obs), _p(pre), K, None, None, None, kind, None, _p(out))


def _rc_tangent(env, K=1, kind=0, hist=None):
    return env._h.lib.pic_tape_tangent_policy(env._h._h, K, None, None, None, None, None, kind, _p(hist), *([None] * 6))


def _err(env):
    return env._h.lib.pic_last_error(env._h._h).decode()


def test_contract():
    from ocplasma_amd._abi import PicError
    Ng, Mo, E = 33, 2, 2
    widths = [2 * Mo, 7, 2 * M]
    pol = _policy(widths, "tanh", hm.make_params(widths, 1), squash=True)
    obs, pre = (np.random.default_rng(s).normal(size=(E, n)) for s, n in ((1, 2 * Mo), (2, 2 * M)))
    env = _make(E, 1000, Ng)
    spec, keep = _spec(env, pol)
    # PIC_ESTATE: the tape entry without a tape; the stand-alone entry without an actuator (it needs no reset and no tape)
    assert _rc_tangent(env) == ESTATE and "no tape is open" in _err(env)
    fresh = _make(E, 1000, Ng, reset=False)
    assert _rc_jvp(fresh, spec, obs, pre) == 0
    fresh.close()
    bare = _make(E, 1000, Ng, actuator=False)
    assert _rc_jvp(bare, spec, obs, pre) == ESTATE and "pic_set_actuator" in _err(bare)
    bare.close()
    # a tape without policy steps
    env.start_tape(4)
    env.step_actions_traj(np.zeros((1, E, 2 * M)))
    before = _state(env)
    assert _rc_tangent(env) == EINVAL and "no steps of pic_tape_step_policy" in _err(env)
    with pytest.raises(PicError, match="no steps of tape_step_policy"):
        env.tangent_policy()
    env.stop_tape()
    # PIC_EINVAL with a reason, nothing enqueued: state, tape length and the tape's bytes untouched
    env.reset(*_start(E, 1000, 1))
    env.start_tape(4)
    env.tape_step_policy(pol, 2)
    before, stats = _state(env), env.tape_stats()
    out = np.full((8, E, 2 * M), 7.0)

    def untouched():
        st = env.tape_stats()
        return _same(_state(env), before) and st["steps"] == stats["steps"] and st["bytes"] == stats["bytes"] and np.all(out == 7.0)

    def refused(reason, K=1, kind=0, **fields):
        s, keep = _spec(env, pol)
        for k, v in fields.items():
            if k.startswith("width"):
                s.width[int(k[5:])] = v
            else:
                setattr(s, k, v)
        rc = _rc_jvp(env, s, obs, pre, K, kind, out)
        assert rc == EINVAL and reason in _err(env), (fields, K, kind, rc, _err(env))
        assert untouched(), (fields, K, kind)

    refused("n_layers", n_layers=0)
    refused("n_layers", n_layers=5)
    refused("width", width1=257)
    refused("width", width1=0)
    refused("width[0]", width0=2 * Mo + 2)
    refused("width[0]", obs_modes=Mo + 1)
    refused("last width", width2=2 * M + 2)
    refused("last width", n_layers=1)
    refused("obs_modes", obs_modes=Ng, width0=2 * Ng)
    refused("obs_modes", obs_modes=65, width0=130)
    refused("mem_kind", kind=2)
    refused("activation", activation=2)
    refused("squash", squash=2)
    refused("per_env", per_env=2)
    refused("params", params=None)
    refused("1 <= K <= 8", K=0)
    refused("1 <= K <= 8", K=9)
    assert _rc_jvp(env, spec, obs, None) == EINVAL and "squash" in _err(env)            # pre NULL with squash
    assert _rc_jvp(env, spec, None, pre) == EINVAL and "obs" in _err(env)
    assert _rc_jvp(env, spec, obs, pre, 8, 0, out) == 0 and _same(_state(env), before)  # allowed under a tape
    assert not np.any(out == 7.0)
    hist = np.full((9, 2, 3, E), 7.0)
    for K, kind, reason in ((0, 0, "1 <= K <= 8"), (9, 0, "1 <= K <= 8"), (1, 2, "mem_kind")):
        assert _rc_tangent(env, K, kind, hist) == EINVAL and reason in _err(env), (K, kind, _err(env))
        st = env.tape_stats()
        assert _same(_state(env), before) and st["steps"] == 2 and st["bytes"] == stats["bytes"] and np.all(hist == 7.0)
    # the call abandons a live walk (the state rules of 7n)
    w = env.walk(Mo)
    w.step(d_energies=np.ones((3, E)))
    assert _rc_tangent(env, 1, 0, hist) == 0 and np.isfinite(hist[0]).all() and _same(_state(env), before)
    with pytest.raises(PicError):
        w.step(d_energies=np.ones((3, E)))
    # the three older tangent entries keep refusing a tape with policy steps
    for call in (lambda: env.tangent(d_actions=np.zeros((2, E, 2 * M))), lambda: env.tangent_walk(K=1),
                 lambda: env.tangent_feedback(d_actions=np.zeros((2, E, 2 * M)))):
        with pytest.raises(PicError, match="error -1: .*policy steps are not built in forward mode"):
            call()
    env.stop_tape()
    # PIC_ENOMEM under a budget that holds the tape and its policy record but not the tangent's working rows
    env.reset(*_start(E, 1000, 1))
    env.start_tape(4)
    env.tape_step_policy(pol, 2)
    need = env.tape_stats()["bytes"]
    env.tangent_policy(d_params=np.ones(pol.n_params))
    grown = env.tape_stats()["bytes"]
    assert grown > need                                                # the working rows count in pic_tape_info.bytes
    env.stop_tape()
    for budget in (need, grown - 256):
        env.reset(*_start(E, 1000, 1))
        env.start_tape(4, budget_bytes=budget)
        env.tape_step_policy(pol, 2)
        x0 = _state(env)
        hist[:] = 7.0
        assert _rc_tangent(env, 1, 0, hist) == ENOMEM and "budget_bytes" in _err(env), _err(env)
        assert env.tape_stats()["steps"] == 2 and _same(_state(env), x0) and np.all(hist == 7.0)
        env.stop_tape()
    env.reset(*_start(E, 1000, 1))
    env.start_tape(4, budget_bytes=grown)
    env.tape_step_policy(pol, 2)
    assert _rc_tangent(env, 1, 0, hist) == 0 and env.tape_stats()["bytes"] == grown
    env.stop_tape()
    env.close()
