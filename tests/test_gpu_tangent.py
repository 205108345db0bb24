"""Forward mode of the tape on the device (pic_tape_tangent): the Jacobian-vector product against torch forward-mode
AD of the restatement (tests/hp_tangent.py), duality with the device's own adjoint, finite differences of the device's rollouts,
bitwise reproducibility, no perturbation of the handle or of a later backward, the C contract and torch forward AD."""
import numpy as np
import pytest

import hp_tangent as ht
import hp_adjoint as ha
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
PARITY_BOUND = 6.2e-11        # 100 x the largest relative error measured against the oracle, 6.2e-13 (ceiling 1e-9)
DUALITY_BOUND = 1.25e-11      # 100 x the largest relative gap measured, 1.25e-13 (ceiling 1e-10)


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


def _actions(T, E, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (T, E, 2 * M))


def _ext_of(actions, Ng):
    lead = actions.shape[:-1]
    flat = actions.reshape(-1, 2 * M)
    out = np.stack([po.actuator_field(L, Ng, M, a[:M], a[M:]).ravel() for a in flat])
    return out.reshape(lead + (Ng,))


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _hist(out):
    return np.stack([out["KE"], out["PE"], out["PE_reward"]], axis=-2)       # [..., T, 3, E]


@pytest.mark.parametrize("E,N,Ng,Ts", [(4, 3000, 64, (1, 5, 20)), (2, 20000, 250, (5, 20)), (1, 40000, 128, (5,))])
def test_tangent_matches_torch_forward_mode(E, N, Ng, Ts):
    for T in Ts:
        env, X, V = _make(E, N, Ng, seed=T)
        x0, v0 = env.particles()
        rng = np.random.default_rng(100 + T)
        a = _actions(T, E, T)
        dx0, dv0 = rng.standard_normal((E, N)), rng.standard_normal((E, N))
        de = 0.1 * rng.standard_normal((T, E, Ng))
        da = rng.standard_normal((T, E, 2 * M))
        env.start_tape(T)
        env.step_actions_traj(a)
        # four directions in one call: x0 alone, v0 alone, raw e_t alone, all three together
        K4 = {"d_x0": np.stack([dx0, 0 * dx0, 0 * dx0, dx0]), "d_v0": np.stack([0 * dv0, dv0, 0 * dv0, dv0]),
              "d_ext": np.stack([0 * de, 0 * de, de, de])}
        out = env.tangent(fields=True, **K4)
        outa = env.tangent(d_actions=da, fields=True)                 # the actions' tangents through the actuator
        st = env.tape_stats()
        env.stop_tape()
        assert st["replay_mismatches"] == 0 and st["replay_bad_positions"] == 0, st
        S = ha.Setup(N, Ng, L, 1.0, env.dt)
        ext = _ext_of(a, Ng)
        dea = _ext_of(da, Ng)
        worst = 0.0
        for e in range(E):
            for k in range(4):
                h, x, v, m = ht.torch_jvp(x0[e], v0[e], ext[:, e], S, K4["d_ext"][k][:, e], K4["d_x0"][k][e], K4["d_v0"][k][e])
                errs = [_rel(_hist(out)[k][:, :, e], h), _rel(out["x"][k][e], x), _rel(out["v"][k][e], v),
                        _rel(out["E_mesh"][k][:, e], m)]
                worst = max(worst, *errs)
            h, x, v, m = ht.torch_jvp(x0[e], v0[e], ext[:, e], S, dea[:, e])
            worst = max(worst, _rel(_hist(outa)[:, :, e], h), _rel(outa["x"][e], x), _rel(outa["v"][e], v),
                        _rel(outa["E_mesh"][:, e], m))
        record_measure(f"tangent.parity.E{E}_N{N}_Ng{Ng}_T{T}", worst)
        assert worst < PARITY_BOUND, worst
        env.close()


@pytest.mark.parametrize("E,N,Ng,T", [(3, 3000, 64, 7), (2, 20000, 250, 12)])
def test_tangent_is_dual_to_the_device_adjoint(E, N, Ng, T):
    """<pic_tape_tangent(u), w> = <u, pic_tape_backward(w)> on the same tape, over every input and output."""
    env, X, V = _make(E, N, Ng, seed=30 + T)
    rng = np.random.default_rng(T)
    env.start_tape(T, 3)
    env.step_actions_traj(_actions(T, E, T))
    de, dx, dv = 0.1 * rng.standard_normal((T, E, Ng)), rng.standard_normal((E, N)), rng.standard_normal((E, N))
    cot, cx, cv = rng.standard_normal((T, 3, E)), rng.standard_normal((E, N)), rng.standard_normal((E, N))
    out = env.tangent(d_ext=de, d_x0=dx, d_v0=dv)
    g = env._h.tape_backward(cot, cx, cv, ext=True, particles=True)
    env.stop_tape()
    worst = 0.0
    for e in range(E):
        lhs = float((_hist(out)[:, :, e] * cot[:, :, e]).sum() + (out["x"][e] * cx[e]).sum() + (out["v"][e] * cv[e]).sum())
        rhs = float((de[:, e] * g["g_ext"][:, e]).sum() + (dx[e] * g["g_x0"][e]).sum() + (dv[e] * g["g_v0"][e]).sum())
        worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    record_measure(f"tangent.duality.E{E}_N{N}_Ng{Ng}_T{T}", worst)
    assert worst < DUALITY_BOUND, worst
    env.close()


def test_directional_derivative_matches_device_finite_differences():
    E, N, Ng, T = 2, 5000, 64, 10
    env, X, V = _make(E, N, Ng, seed=3)
    a = _actions(T, E, 3)
    rng = np.random.default_rng(9)
    da = rng.standard_normal((3, T, E, 2 * M))
    env.start_tape(T)
    env.step_actions_traj(a)
    out = env.tangent(d_actions=da)
    env.stop_tape()
    eps = 1e-6
    worst = 0.0
    for k in range(3):
        env.reset(X, V)
        _, _, pp = env.step_actions_traj(a + eps * da[k], history=True)
        env.reset(X, V)
        _, _, pm = env.step_actions_traj(a - eps * da[k], history=True)
        fd = (pp.sum() - pm.sum()) / (2 * eps)
        an = float(out["PE_reward"][k].sum())
        worst = max(worst, abs(fd - an) / abs(an))
    record_measure("tangent.fd_rel_eps1e-6", worst)
    assert worst < 6.9e-6, worst         # 100 x the 6.9e-8 measured at eps = 1e-6 (ceiling 1e-5)
    env.close()


def test_k_directions_equal_k_calls():
    E, N, Ng, T = 3, 4000, 64, 6
    env, X, V = _make(E, N, Ng, seed=5)
    rng = np.random.default_rng(5)
    env.start_tape(T, 2)
    env.step_actions_traj(_actions(T, E, 5))
    for K in (3, 8):
        de = 0.1 * rng.standard_normal((K, T, E, Ng))
        dx, dv = rng.standard_normal((K, E, N)), rng.standard_normal((K, E, N))
        many = env.tangent(d_ext=de, d_x0=dx, d_v0=dv, fields=True)
        for k in range(K):
            one = env.tangent(d_ext=de[k], d_x0=dx[k], d_v0=dv[k], fields=True)
            for key in one:
                assert np.array_equal(many[key][k], one[key]), (K, k, key)
    env.stop_tape()
    env.close()


def test_tangent_is_bitwise_reproducible():
    E, N, Ng, T = 3, 3000, 64, 7
    a = _actions(T, E, 2)
    rng = np.random.default_rng(2)
    de = 0.1 * rng.standard_normal((2, T, E, Ng))
    dx, dv = rng.standard_normal((2, E, N)), rng.standard_normal((2, E, N))

    def run(every=0, **kw):
        env, X, V = _make(E, N, Ng, seed=2, **kw)
        env.start_tape(T, every)
        env.step_actions_traj(a)
        out = env.tangent(d_ext=de, d_x0=dx, d_v0=dv, fields=True)
        sched = env._h.schedule()
        env.stop_tape()
        env.close()
        return out, sched

    ref, s0 = run()
    assert s0 == "resident"
    variants = [run()[0], run(blocks_per_env=1)[0], run(blocks_per_env=-1)[0]]
    o2, s2 = run(blocks_per_env=2)
    assert s2 == "streaming"
    variants += [o2] + [run(every=k)[0] for k in (1, 3, T)]
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
    one.start_tape(T)
    one.step_actions_traj(a[:, 1:2])
    alone = one.tangent(d_ext=de[:, :, 1:2], d_x0=dx[:, 1:2], d_v0=dv[:, 1:2], fields=True)
    one.stop_tape()
    for k in ("KE", "PE", "PE_reward", "E_mesh"):
        assert np.array_equal(alone[k][:, :, 0], ref[k][:, :, 1]), k
    for k in ("x", "v"):
        assert np.array_equal(alone[k][:, 0], ref[k][:, 1]), k
    one.close()


@pytest.mark.parametrize("blocks", [0, 2])
def test_tangent_leaves_the_handle_and_the_backward_alone(blocks):
    E, N, Ng, T = 2, 3000, 64, 6
    a = _actions(T, E, 4)
    rng = np.random.default_rng(4)
    envs = [_make(E, N, Ng, seed=4, blocks_per_env=blocks)[0] for _ in range(3)]
    taped, twin, plain = envs
    for env in (taped, twin):
        env.start_tape(T, 2)
    for env in envs:
        env.step_actions_traj(a)
    before = [np.copy(u) for u in taped.particles() + taped.fields() + taped.energies()]
    taped.tangent(d_actions=rng.standard_normal((4, T, E, 2 * M)), d_x0=rng.standard_normal((4, E, N)), fields=True)
    st = taped.tape_stats()
    assert st["replay_mismatches"] == 0 and st["replay_bad_positions"] == 0 and st["steps"] == T, st
    for u, w in zip(taped.particles() + taped.fields() + taped.energies(), before):
        assert np.array_equal(u, w)
    cot = rng.standard_normal((T, E))
    g1 = taped.backward(d_PE_reward=cot, d_x=np.ones((E, N)))
    g2 = twin.backward(d_PE_reward=cot, d_x=np.ones((E, N)))
    for k in g2:
        assert np.array_equal(g1[k], g2[k]), k
    taped.stop_tape()
    twin.stop_tape()
    for env in (taped, plain):
        env.step_actions(a[0], 3)
    for u, w in zip(taped.particles() + taped.fields() + taped.energies(), plain.particles() + plain.fields() + plain.energies()):
        assert np.array_equal(u, w)
    for env in envs:
        env.close()


def test_tangent_contract():
    from ocplasma_amd._abi import PicError
    env, X, V = _make(1, 2000, 64, seed=6)
    h = env._h
    with pytest.raises(PicError, match="-3"):
        h.tape_tangent(1)                                            # no tape
    env.start_tape(4, 2)
    # T = 0: the initial tangents pass through
    dx, dv = np.random.default_rng(1).standard_normal((2, 1, 2000)), np.random.default_rng(2).standard_normal((2, 1, 2000))
    out = h.tape_tangent(2, d_x0=dx, d_v0=dv)
    assert np.array_equal(out["x"], dx) and np.array_equal(out["v"], dv) and out["hist"].size == 0
    env.step_actions(_actions(1, 1, 6)[0], 4)
    for K in (0, 9):
        with pytest.raises(PicError, match="-1"):
            h.tape_tangent(K)
    with pytest.raises(PicError, match="-1"):
        h.tape_tangent(1, d_ext=np.zeros((1, 4, 1, 64)), d_actions=np.zeros((1, 4, 1, 2 * M)))
    # a walk in progress is abandoned
    w = env.walk()
    w.step()
    env.tangent(d_x0=np.ones((1, 2000)))
    with pytest.raises(PicError, match="-3"):
        w.step()
    # a tight budget: PIC_ENOMEM, and the tape still backwards
    env.stop_tape()
    env.reset(X, V)
    env.start_tape(4, 2)
    tight = env.tape_stats()["bytes"] + 1024
    env.stop_tape()
    env.reset(X, V)
    env.start_tape(4, 2, budget_bytes=tight)
    env.step(None, 4)
    with pytest.raises(PicError, match="-4"):
        h.tape_tangent(1, d_x0=np.ones((1, 1, 2000)))
    g = env.backward(d_PE_reward=np.ones((4, 1)))
    assert np.all(np.isfinite(g["x0"])) and env.tape_stats()["replay_mismatches"] == 0
    env.stop_tape()
    env.close()
    # d_actions without an actuator
    e2, X2, V2 = _make(1, 2000, 64, seed=7, actuator=False)
    e2.start_tape(2)
    e2.step(None, 2)
    with pytest.raises(PicError, match="-3"):
        e2._h.tape_tangent(1, d_actions=np.zeros((1, 2, 1, 2)))
    e2.stop_tape()
    e2.close()
    # a gain-law tape is refused with the reason
    import hp_feedback as hf
    e3, _, _ = _make(1, 2000, 64, seed=8)
    e3.start_tape(3)
    e3.step_feedback_gain(hf.g0(M), 3)
    with pytest.raises(PicError, match="gain law"):
        e3._h.tape_tangent(1, d_x0=np.ones((1, 1, 2000)))
    e3.stop_tape()
    e3.close()


def test_torch_forward_ad_matches_tangent_and_passes_gradcheck():
    import torch
    import torch.autograd.forward_ad as fwAD
    from ocplasma_amd.env import grad
    E, N, Ng, T = 2, 3000, 64, 5
    env, X, V = _make(E, N, Ng, seed=8)
    a = torch.tensor(_actions(T, E, 8), dtype=torch.float64, device="cuda")
    du = torch.tensor(np.random.default_rng(8).standard_normal((T, E, 2 * M)), dtype=torch.float64, device="cuda")
    with fwAD.dual_level():
        outs = grad.rollout(env, fwAD.make_dual(a, du))
        tans = [fwAD.unpack_dual(o).tangent for o in outs]
        prim = [fwAD.unpack_dual(o).primal for o in outs]
    ref = env.tangent(d_actions=du)
    for t, k in zip(tans, ("KE", "PE", "PE_reward")):
        assert torch.equal(t, ref[k]), k
    env.stop_tape()
    env.reset(X, V)
    ke, pe, per = grad.rollout(env, a)                               # the primal outputs are unchanged
    for u, w in zip(prim, (ke, pe, per)):
        assert torch.equal(u, w)
    env.stop_tape()
    # raw fields
    env.reset(X, V)
    e = torch.tensor(0.05 * np.random.default_rng(14).standard_normal((4, E, Ng)), dtype=torch.float64, device="cuda")
    de = torch.tensor(np.random.default_rng(15).standard_normal((4, E, Ng)), dtype=torch.float64, device="cuda")
    with fwAD.dual_level():
        tans = [fwAD.unpack_dual(o).tangent for o in grad.rollout_ext(env, fwAD.make_dual(e, de))]
    ref = env.tangent(d_ext=de)
    for t, k in zip(tans, ("KE", "PE", "PE_reward")):
        assert torch.equal(t, ref[k]), k
    env.stop_tape()
    env.close()

    def f(u):
        env, _, _ = _make(2, 500, 32, seed=9)
        return grad.rollout(env, u)
    u = torch.tensor(_actions(3, 2, 9), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(f, (u,), eps=1e-6, atol=1e-6, rtol=1e-4, check_forward_ad=True, check_backward_ad=False,
                                    check_undefined_grad=False, check_batched_grad=False)
