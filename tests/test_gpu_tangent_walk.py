"""Forward mode through closed loops on the device (pic_tape_tangent_walk_*, pic_tape_tangent_feedback): the walk
against pic_tape_tangent bit for bit on open-loop tapes, the modes' tangents against J dE, the gain law against torch forward-mode
AD of the restatement (tests/hp_feedback.py), duality with the device's reverse passes (backward_feedback, rollout_policy), bitwise
invariants, torch forward AD of rollout_feedback, and the C contract."""
import numpy as np
import pytest

import hp_adjoint as ha
import hp_feedback as hf
import hp_policy as hpp
import hp_tangent as ht
import hp_tangent_walk as hw
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
MODES_BOUND = 1e-12           # two summation orders of <= 250 float64 terms
PARITY_BOUND = 2.3e-11        # 100 x the largest relative error measured against the oracle, 2.21e-13 (ceiling 1e-9)
DUALITY_BOUND = 3.7e-12       # 100 x the largest relative gap measured, 3.68e-14 (ceiling 1e-10)


def _make(E, N, Ng, seed=1, actuator=True, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    X = np.empty((E, N))
    V = np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=seed + 7 * e)
    env.reset(X, V)
    if actuator:
        env.set_actuator(oc.E_field(L, Ng, M))
    return env, X, V


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _same(a, b):
    a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _gain(E, seed):
    return hf.g0(M)[None] + np.random.default_rng(seed).uniform(-0.3, 0.3, (E, 2 * M, 2 * M))


def _walk_all(env, T, K=None, obs_modes=0, d_x0=None, d_v0=None, d_gain=None, d_actions=None, d_ext=None, on_device=False):
    """A whole walk, row s of d_actions / d_ext [K, T, ...] at step s: dict of stacked per-step outputs [K, T, ...]."""
    w = env.tangent_walk(K=K, obs_modes=obs_modes, d_x0=d_x0, d_v0=d_v0, d_gain=d_gain, on_device=on_device)
    rows = []
    for s in range(T):
        r = w.step(d_actions=None if d_actions is None else d_actions[:, s], d_ext=None if d_ext is None else d_ext[:, s],
                   fields=True)
        assert r.pop("t") == s
        rows.append(r)
    out = {k: np.stack([_np(r[k]) for r in rows], axis=1) for k in rows[0]} if rows else {}
    out["x"], out["v"] = (_np(a) for a in w.end())
    if w.d_modes0 is not None:
        out["modes0"] = _np(w.d_modes0)
    return out


# ---- 1. open loop: the walk is pic_tape_tangent ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E,N,Ng,every", [("actions", 3, 3000, 64, 3), ("ext", 1, 1000, 250, 1), ("actions", 1, 100001, 32, 3)])
def test_open_loop_walk_is_tape_tangent_bit_for_bit(kind, E, N, Ng, every):
    T = 7 if N < 100000 else 2
    env, X, V = _make(E, N, Ng, seed=2)
    rng = np.random.default_rng(N)
    env.start_tape(T, every)
    if kind == "actions":
        env.step_actions_traj(rng.uniform(-0.5, 0.5, (T, E, 2 * M)))
    else:
        env.step_ext_traj(0.05 * rng.standard_normal((T, E, Ng)))
    for K in ((1, 3, 8) if N < 100000 else (3,)):
        u = rng.standard_normal((K, T, E, 2 * M)) if kind == "actions" else 0.1 * rng.standard_normal((K, T, E, Ng))
        dx, dv = rng.standard_normal((K, E, N)), rng.standard_normal((K, E, N))
        key = "d_" + kind
        want = env.tangent(d_x0=dx, d_v0=dv, fields=True, **{key: u})
        for on_device in (False, True):
            got = _walk_all(env, T, K=K, d_x0=dx, d_v0=dv, on_device=on_device, **{key: u})
            st = env.tape_stats()
            assert st["replay_mismatches"] == 0 and st["replay_bad_positions"] == 0, st
            for k in ("KE", "PE", "PE_reward", "E_mesh", "x", "v"):
                assert _same(got[k], want[k]), (K, on_device, k)
        if kind == "actions":
            one = env.tangent_feedback(d_actions=u, d_x0=dx, d_v0=dv, fields=True)
            for k in ("KE", "PE", "PE_reward", "E_mesh", "x", "v"):
                assert _same(one[k], want[k]), (K, k)
            assert _same(one["actions"], u) and not np.any(one["modes"])
    env.stop_tape()
    env.close()


# ---- 2. the modes' tangents ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,Ng,Mo", [(3, 1000, 64, 5), (1, 3000, 250, 2), (1, 1000, 32, 31)])
def test_modes_tangents_are_the_jacobian_of_the_field_tangents(E, N, Ng, Mo):
    T, K = 4, 3
    env, X, V = _make(E, N, Ng, seed=3)
    rng = np.random.default_rng(Ng)
    x0, _ = env.particles()
    env.start_tape(T, 3)
    env.step_actions_traj(rng.uniform(-0.5, 0.5, (T, E, 2 * M)))
    da, dx, dv = rng.standard_normal((K, T, E, 2 * M)), rng.standard_normal((K, E, N)), rng.standard_normal((K, E, N))
    out = _walk_all(env, T, K=K, obs_modes=Mo, d_x0=dx, d_v0=dv, d_actions=da)
    env.stop_tape()
    J = hf.jacobian(Ng, Mo)
    S = ha.Setup(N, Ng, L, 1.0, env.dt)
    worst = _rel(out["modes"], np.einsum("mj,ktej->ktem", J, out["E_mesh"]))
    for k in range(K):
        for e in range(E):
            dE0 = ha._np_K(ht._tangent_deposit(dx[k, e], x0[e], S), S)
            worst = max(worst, _rel(out["modes0"][k, e], J @ dE0))
    record_measure(f"tangent_walk.modes.E{E}_N{N}_Ng{Ng}_Mo{Mo}", worst)
    assert worst < MODES_BOUND, worst
    env.close()


# ---- 3. the gain law against torch forward mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,Ng,T,every", [(3, 1000, 32, 4, 3), (1, 3000, 64, 7, 3), (1, 3000, 250, 7, 1)])
def test_gain_law_matches_torch_forward_mode(E, N, Ng, T, every):
    K = 2
    env, X, V = _make(E, N, Ng, seed=4)
    rng = np.random.default_rng(T + Ng)
    G = _gain(E, Ng)
    dG = rng.standard_normal((K, E, 2 * M, 2 * M))
    dx, dv = rng.standard_normal((K, E, N)), rng.standard_normal((K, E, N))
    X, V = env.particles()
    env.start_tape(T, every)
    env.step_feedback_gain(G, T)
    one = env.tangent_feedback(d_gain=dG, d_x0=dx, d_v0=dv, fields=True)
    for on_device in (False, True):
        got = _walk_all(env, T, K=K, d_gain=dG, d_x0=dx, d_v0=dv, on_device=on_device)
        for k in ("KE", "PE", "PE_reward", "E_mesh", "x", "v", "actions"):
            assert _same(got[k], one[k]), (on_device, k)
    assert env.tape_stats()["replay_mismatches"] == 0
    from ocplasma_amd._abi import PicError
    with pytest.raises(PicError, match="gain law"):
        env.tangent(d_x0=dx)
    env.stop_tape()
    S = ha.Setup(N, Ng, L, 1.0, env.dt)
    worst = 0.0
    for e in range(E):
        for k in range(K):
            th, tm, ta, tx, tv = hw.torch_feedback_jvp(X[e], V[e], G[e], S, T, M, dG[k, e], dx[k, e], dv[k, e])
            hist = np.stack([one["KE"][k, :, e], one["PE"][k, :, e], one["PE_reward"][k, :, e]], -1)
            worst = max(worst, _rel(hist, th), _rel(one["modes"][k, :, e], tm), _rel(one["actions"][k, :, e], ta),
                        _rel(one["x"][k, e], tx), _rel(one["v"][k, e], tv))
    record_measure(f"tangent_walk.parity.E{E}_N{N}_Ng{Ng}_T{T}", worst)
    assert worst < PARITY_BOUND, worst
    env.close()


# ---- 4. duality with the reverse passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,Ng,T,every", [(3, 1000, 64, 7, 3), (1, 3000, 250, 5, 1)])
def test_tangent_feedback_is_dual_to_backward_feedback(E, N, Ng, T, every):
    env, X, V = _make(E, N, Ng, seed=5)
    rng = np.random.default_rng(Ng + T)
    G = _gain(E, T)
    env.start_tape(T, every)
    env.step_feedback_gain(G, T)
    dG, dx, dv = rng.standard_normal((E, 2 * M, 2 * M)), rng.standard_normal((E, N)), rng.standard_normal((E, N))
    cot = {k: rng.standard_normal((T, E)) for k in ("KE", "PE", "PE_reward")}
    cm, cx, cv = rng.standard_normal((T, E, 2 * M)), rng.standard_normal((E, N)), rng.standard_normal((E, N))
    out = env.tangent_feedback(d_gain=dG, d_x0=dx, d_v0=dv)
    g = env.backward(d_KE=cot["KE"], d_PE=cot["PE"], d_PE_reward=cot["PE_reward"], d_x=cx, d_v=cv, d_modes=cm)
    env.stop_tape()
    worst = 0.0
    for e in range(E):
        lhs = float(sum((out[k][:, e] * cot[k][:, e]).sum() for k in cot) + (out["modes"][:, e] * cm[:, e]).sum()
                    + (out["x"][e] * cx[e]).sum() + (out["v"][e] * cv[e]).sum())
        rhs = float((g["gain"][e] * dG[e]).sum() + (g["x0"][e] * dx[e]).sum() + (g["v0"][e] * dv[e]).sum())
        worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    record_measure(f"tangent_walk.duality.E{E}_N{N}_Ng{Ng}_T{T}", worst)
    assert worst < DUALITY_BOUND, worst
    env.close()


@pytest.mark.parametrize("observe", ["modes", "state"])
def test_rollout_policy_jvp_is_dual_to_rollout_policy_backward(observe):
    import torch
    from ocplasma_amd.env import grad
    E, N, Ng, T, K = 3, 1000, 64, 5, 2
    env, X, V = _make(E, N, Ng, seed=6)
    if observe == "modes":
        p0 = hpp.mlp_params(2 * M, 2 * M, 8, seed=3)
        fn = hpp.mlp_modes
    else:
        p0 = hpp.deepsets_params(2 * M, 8, seed=3)
        fn = lambda q, o: hpp.deepsets_state(q, o, L)                                # noqa: E731
    p = {k: t.to("cuda").clone().requires_grad_(True) for k, t in p0.items()}
    g = torch.Generator().manual_seed(9)
    dps = [{k: torch.randn(t.shape, generator=g, dtype=torch.float64).to("cuda") for k, t in p0.items()} for _ in range(K)]
    del dps[1]["b1"]                                                                 # a missing name is zero
    w_hist = torch.randn((3, T, E), generator=g, dtype=torch.float64).to("cuda")
    w_act = torch.randn((T, E, 2 * M), generator=g, dtype=torch.float64).to("cuda")
    ke, pe, per, acts, _ = grad.rollout_policy(env, lambda o: fn(p, o), T, observe=observe, checkpoint_every=3)
    ((torch.stack([ke, pe, per]) * w_hist).sum() + (acts * w_act).sum()).backward()
    env.stop_tape()
    env.reset(X, V)
    with torch.no_grad():
        pd = {k: t.detach() for k, t in p.items()}
    out = grad.rollout_policy_jvp(env, fn, pd, dps, T, observe=observe, checkpoint_every=3)
    assert env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    for a, b in ((out["KE"], ke), (out["PE"], pe), (out["PE_reward"], per), (out["actions"], acts)):
        assert torch.equal(a, b.detach())
    worst = 0.0
    for k in range(K):
        lhs = float((torch.stack([out["dKE"][k], out["dPE"][k], out["dPE_reward"][k]]) * w_hist).sum()
                    + (out["d_actions"][k] * w_act).sum())
        rhs = float(sum((p[name].grad * d).sum() for name, d in dps[k].items()))
        worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    record_measure(f"tangent_walk.policy_duality.{observe}", worst)
    assert worst < DUALITY_BOUND, worst
    env.close()


# ---- 5. bitwise invariants -------------------------------------------------------------------------------------------------------
def test_closed_loop_walk_is_bitwise_reproducible():
    E, N, Ng, T, K = 3, 3000, 64, 7, 3
    rng = np.random.default_rng(7)
    G = _gain(E, 7)
    dG, dx, dv = rng.standard_normal((K, E, 2 * M, 2 * M)), rng.standard_normal((K, E, N)), rng.standard_normal((K, E, N))
    da = rng.standard_normal((K, T, E, 2 * M))

    def run(every=0, envs=slice(None), **kw):
        env, _, _ = _make(E, N, Ng, seed=7, **kw)
        if envs != slice(None):
            x, v = env.particles()
            env.close()
            import ocplasma_amd as oc
            from ocplasma_amd.env.batched import BatchedPIC
            env = BatchedPIC(1, N, Ng, L=L, dt=0.1)
            env.reset(x[envs], v[envs])
            env.set_actuator(oc.E_field(L, Ng, M))
        env.start_tape(T, every)
        env.step_feedback_gain(G[envs], T)
        out = _walk_all(env, T, K=K, obs_modes=2, d_gain=dG[:, envs], d_x0=dx[:, envs], d_v0=dv[:, envs], d_actions=da[:, :, envs])
        again = _walk_all(env, T, K=K, obs_modes=2, d_gain=dG[:, envs], d_x0=dx[:, envs], d_v0=dv[:, envs], d_actions=da[:, :, envs])
        for k in out:
            assert _same(out[k], again[k]), k                          # a second walk repeats the first
        singles = [_walk_all(env, T, K=1, obs_modes=2, d_gain=dG[k:k + 1, envs], d_x0=dx[k:k + 1, envs], d_v0=dv[k:k + 1, envs],
                             d_actions=da[k:k + 1, :, envs]) for k in (range(K) if every == 0 else ())]
        sched = env._h.schedule()
        env.stop_tape()
        env.close()
        return out, sched, singles

    ref, s0, singles = run()
    assert s0 == "resident"
    for k, one in enumerate(singles):                                  # K directions equal K single-direction walks
        for key in ref:
            assert _same(one[key][0], ref[key][k]), (k, key)
    o2, s2, _ = run(every=1, blocks_per_env=2)
    assert s2 == "streaming"
    for out in (o2, run(every=3, blocks_per_env=1)[0]):
        for key in ref:
            assert _same(out[key], ref[key]), key
    alone = run(every=3, envs=slice(1, 2))[0]                          # environment 1 of the batch alone
    for key in ref:
        ax = 1 if key in ("x", "v", "modes0") else 2
        assert _same(alone[key], np.take(ref[key], [1], axis=ax)), key


# ---- 6. torch forward AD of rollout_feedback -------------------------------------------------------------------------------------
def test_rollout_feedback_forward_ad_matches_tangent_feedback_and_passes_gradcheck():
    import torch
    import torch.autograd.forward_ad as fwAD
    from ocplasma_amd.env import grad
    E, N, Ng, T = 2, 1000, 32, 3
    env, X, V = _make(E, N, Ng, seed=8)
    G = torch.tensor(_gain(E, 8), dtype=torch.float64, device="cuda")
    dG = torch.tensor(np.random.default_rng(8).standard_normal((E, 2 * M, 2 * M)), dtype=torch.float64, device="cuda")
    with fwAD.dual_level():
        tans = [fwAD.unpack_dual(o).tangent for o in grad.rollout_feedback(env, fwAD.make_dual(G, dG), T)]
    ref = env.tangent_feedback(d_gain=dG)
    for t, k in zip(tans, ("KE", "PE", "PE_reward", "modes")):
        assert torch.equal(t, ref[k]), k
    env.stop_tape()
    env.close()

    def f(g):
        env, _, _ = _make(E, N, Ng, seed=8)
        return grad.rollout_feedback(env, g, T)
    g = G.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (g,), eps=1e-6, atol=1e-6, rtol=1e-4, check_forward_ad=True, check_backward_ad=False,
                                    nondet_tol=0.0)


# ---- 7. contract -----------------------------------------------------------------------------------------------------------------
def test_tangent_walk_contract():
    from ocplasma_amd._abi import PIC_HOST, PicError
    N, Ng, T = 1000, 32, 3
    env, X, V = _make(1, N, Ng, seed=9)
    h = env._h
    z = lambda *s: np.zeros(s)                                                       # noqa: E731
    begin = lambda K=1, mo=0, gain=None: h.tape_tangent_walk_begin(K, mo, 0, 0, 0 if gain is None else gain.ctypes.data,  # noqa: E731
                                                                   PIC_HOST, 0)
    step = lambda ext=None, act=None: h.tape_tangent_walk_step(0 if ext is None else ext.ctypes.data,  # noqa: E731
                                                               0 if act is None else act.ctypes.data, PIC_HOST, 0, 0, 0, 0, 0, 0)
    with pytest.raises(PicError, match="-3"):
        begin()                                                        # no tape
    env.start_tape(T + 1, 2)
    env.step_actions_traj(np.random.default_rng(9).uniform(-0.5, 0.5, (1, 1, 2 * M)))
    env.step_feedback_gain(hf.g0(M), T - 1)
    for K, mo in ((0, 0), (9, 0), (1, -1), (1, Ng)):
        with pytest.raises(PicError, match="-1"):
            begin(K, mo)
    with pytest.raises(PicError, match="-3"):
        step()                                                         # no live walk
    with pytest.raises(PicError, match="-3"):
        h.tape_tangent_walk_end(PIC_HOST, 0, 0)
    begin()
    with pytest.raises(PicError, match="-1"):
        step(ext=z(1, 1, Ng), act=z(1, 1, 2 * M))                      # both
    assert step(ext=z(1, 1, Ng)) == 0                                  # step 0 is open loop: d_ext is fine
    with pytest.raises(PicError, match="-1"):
        step(ext=z(1, 1, Ng))                                          # step 1 is a law step
    with pytest.raises(PicError, match="-3"):
        h.tape_tangent_walk_end(PIC_HOST, 0, 0)                        # steps left
    assert step() == 1 and step(act=z(1, 1, 2 * M)) == 2
    with pytest.raises(PicError, match="-3"):
        step()                                                         # past T
    h.tape_tangent_walk_end(PIC_HOST, 0, 0)
    with pytest.raises(PicError, match="-3"):
        h.tape_tangent_walk_end(PIC_HOST, 0, 0)                        # ended
    # whatever abandons a tangent walk
    for spoil in (lambda: env.backward(d_PE_reward=np.ones((T, 1))), lambda: env.walk(), lambda: env.step(None, 1)):
        w = env.tangent_walk(obs_modes=2)
        spoil()
        with pytest.raises(PicError):
            w.step()
    assert env.tape_stats()["steps"] == T + 1
    # a tangent walk abandons a reverse walk
    r = env.walk()
    env.tangent_walk()
    with pytest.raises(PicError):
        r.step()
    with pytest.raises(PicError, match="gain law"):
        h.tape_tangent(1, d_x0=np.ones((1, 1, N)))
    env.stop_tape()
    # d_gain on a tape without a law step
    env.reset(X, V)
    env.start_tape(2)
    env.step(None, 2)
    with pytest.raises(PicError, match="-1"):
        begin(gain=z(1, 1, 2 * M, 2 * M))
    env.stop_tape()
    env.close()
    # d_actions without an actuator
    e2, _, _ = _make(1, N, Ng, seed=10, actuator=False)
    e2.start_tape(2)
    e2.step(None, 2)
    e2._h.tape_tangent_walk_begin(1, 0, 0, 0, 0, PIC_HOST, 0)
    with pytest.raises(PicError, match="-3"):
        e2._h.tape_tangent_walk_step(0, z(1, 1, 2).ctypes.data, PIC_HOST, 0, 0, 0, 0, 0, 0)
    e2.stop_tape()
    e2.close()


@pytest.mark.parametrize("blocks", [0, 2])
def test_tangent_walk_leaves_the_handle_and_the_backward_alone(blocks):
    E, N, Ng, T = 3, 3000, 64, 6
    rng = np.random.default_rng(11)
    G = _gain(E, 11)
    taped, twin = (_make(E, N, Ng, seed=11, blocks_per_env=blocks)[0] for _ in range(2))
    for env in (taped, twin):
        env.start_tape(T, 2)
        env.step_feedback_gain(G, T)
    before = [np.copy(u) for u in taped.particles() + taped.fields() + taped.energies()]
    _walk_all(taped, T, K=4, obs_modes=M, d_gain=rng.standard_normal((4, E, 2 * M, 2 * M)), d_x0=rng.standard_normal((4, E, N)))
    taped.tangent_feedback(d_gain=rng.standard_normal((E, 2 * M, 2 * M)))
    st = taped.tape_stats()
    assert st["replay_mismatches"] == 0 and st["replay_bad_positions"] == 0 and st["steps"] == T, st
    for u, w in zip(taped.particles() + taped.fields() + taped.energies(), before):
        assert np.array_equal(u, w)
    cot, cm = rng.standard_normal((T, E)), rng.standard_normal((T, E, 2 * M))
    g1 = taped.backward(d_PE_reward=cot, d_x=np.ones((E, N)), d_modes=cm)
    g2 = twin.backward(d_PE_reward=cot, d_x=np.ones((E, N)), d_modes=cm)
    for k in g2:
        assert np.array_equal(g1[k], g2[k]), k
    for env in (taped, twin):
        env.stop_tape()
        env.close()
