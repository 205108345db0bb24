"""The gain law a_t = G m_t on the device (pic_step_feedback_gain): G0 against pic_step_feedback bit for bit,
a random G against the host loop, and the closed-loop gradient (pic_tape_backward_feedback) against torch autograd of the
restatement (tests/hp_feedback.py), finite differences, bitwise reproducibility and the C contract."""
import numpy as np
import pytest

import hp_adjoint as ha
import hp_feedback as hf
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
PARITY_BOUND = 3e-12          # 100 x the largest relative error measured against autograd, 2.6e-14 (feedback_gain_grad_rel_err_*)


def _make(E, N, Ng, seed=1, M_=M, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    X = np.empty((E, N))
    V = np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=seed + 7 * e)
    env.reset(X, V)
    env.set_actuator(oc.E_field(L, Ng, M_))
    return env, X, V


def _state(env):
    x, v = env.particles()
    return [np.asarray(a).copy() for a in (x, v, *env.fields(), *env.energies())]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _random_gain(E, n, seed, scale=0.4):
    return np.random.default_rng(seed).uniform(-scale, scale, (E, n, n))


CASES = [(dtype, pos, shape, scheme, bpe)
         for dtype, pos in (("float64", None), ("float32", None), ("float32", "fixed32"))
         for shape in ("CIC", "TSC")
         for scheme in ("symplectic_4th_order", "verlet")
         for bpe in (0, 2)]


@pytest.mark.parametrize("dtype,pos,shape,scheme,bpe", CASES)
def test_g0_is_step_feedback_bit_for_bit(dtype, pos, shape, scheme, bpe):
    E, N, Ng, T, M_ = 2, 5000, 250, 6, 5
    kw = dict(dtype=dtype, position_dtype=pos, interpol=shape, integrator=scheme, blocks_per_env=bpe)
    a, _, _ = _make(E, N, Ng, M_=M_, **kw)
    b, _, _ = _make(E, N, Ng, M_=M_, **kw)
    assert a._h.schedule() == ("resident" if bpe == 0 else "streaming")
    ra = a.step_feedback(T, actions=True, history=True)
    rb = b.step_feedback_gain(hf.g0(M_), T, actions=True, modes=True, history=True)
    for k in ("actions", "KE", "PE", "PE_reward"):
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(rb["actions"], np.concatenate([-rb["modes"][..., :M_], rb["modes"][..., M_:]], -1))
    assert _same(_state(a), _state(b))
    # a second call continues from the field the first one left
    a.step_feedback(2)
    b.step_feedback_gain(hf.g0(M_), 2)
    assert _same(_state(a), _state(b))
    a.close()
    b.close()


@pytest.mark.parametrize("bpe", [0, 2])
def test_g0_bit_for_bit_with_recorder(bpe):
    E, N, Ng, T, M_ = 2, 5000, 250, 7, 5
    outs = []
    for gain in (None, hf.g0(M_)):
        env, _, _ = _make(E, N, Ng, M_=M_, blocks_per_env=bpe)
        env.start_recording(stride=3, modes=4, x_bins=16)
        r = env.step_feedback(T, actions=True) if gain is None else env.step_feedback_gain(gain, T, actions=True)
        rec = env.recorded()
        outs.append((r["actions"], _state(env), rec))
        env.close()
    (a0, s0, r0), (a1, s1, r1) = outs
    assert np.array_equal(a0, a1) and _same(s0, s1)
    for k in ("steps", "KE", "PE", "Ek", "x_hist"):
        assert np.array_equal(np.asarray(getattr(r0, k)), np.asarray(getattr(r1, k))), k


@pytest.mark.parametrize("bpe", [0, 2])
def test_random_gain_is_the_host_loop(bpe):
    E, N, Ng, T, M_ = 3, 5000, 250, 5, 4
    n = 2 * M_
    G = _random_gain(E, n, 11)
    G[0, 1, :] = 0.0                 # a row without a non-zero entry: +0
    G[1, :, 2] = 0.0
    dev, _, _ = _make(E, N, Ng, M_=M_, blocks_per_env=bpe)
    host, _, _ = _make(E, N, Ng, M_=M_, blocks_per_env=bpe)
    r = dev.step_feedback_gain(G, T, actions=True, modes=True)
    for t in range(T):
        ek = host.modes(M_)
        m = np.concatenate([ek.real, ek.imag], axis=1)
        assert np.array_equal(m, r["modes"][t]), t
        act = np.stack([hf.law_action(G[e], m[e]) for e in range(E)])
        assert np.array_equal(act, r["actions"][t]), t
        host.step_actions(act)
    assert _same(_state(dev), _state(host))
    # the torch form: a device tensor, and [2M, 2M] for every environment
    import torch
    d2, _, _ = _make(E, N, Ng, M_=M_, blocks_per_env=bpe)
    d3, _, _ = _make(E, N, Ng, M_=M_, blocks_per_env=bpe)
    r2 = d2.step_feedback_gain(torch.as_tensor(G[2], device="cuda"), T, actions=True)
    r3 = d3.step_feedback_gain(np.broadcast_to(G[2], (E, n, n)), T, actions=True)
    assert np.array_equal(r2["actions"], r3["actions"]) and _same(_state(d2), _state(d3))
    for env in (dev, host, d2, d3):
        env.close()


def _taped(env, gain, T, every, cot_hist, cot_modes=None, cot_x=None, cot_v=None):
    env.start_tape(T, every)
    fwd = env.step_feedback_gain(gain, T, actions=True, modes=True)
    out = env._h.tape_backward_feedback(cot_hist, cot_x, cot_v, cot_modes)
    st = env.tape_stats()
    env.stop_tape()
    assert st["replay_mismatches"] == 0 and st["unit_retries"] == 0, st
    return fwd, out


def _gain_grad(out, first=0, k=None):
    a, m = out["g_actions"], out["modes"]
    k = a.shape[0] - first if k is None else k
    return sum(a[s][:, :, None] * m[s][:, None, :] for s in range(first, first + k))


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


@pytest.mark.parametrize("bpe", [0, 2])
@pytest.mark.parametrize("E", [1, 3])
def test_gradients_match_autograd(E, bpe):
    N, Ng = 3000, 64
    n = 2 * M
    worst = 0.0
    for T in (1, 5, 20):
        for every in (0, 2):
            env, _, _ = _make(E, N, Ng, seed=T, blocks_per_env=bpe)
            x0, v0 = env.particles()
            x0, v0 = np.asarray(x0).copy(), np.asarray(v0).copy()
            rng = np.random.default_rng(T + every)
            G = np.stack([hf.g0(M) + 0.3 * rng.standard_normal((n, n)) for _ in range(E)])
            cot = rng.standard_normal((T, 3, E))
            cm = rng.standard_normal((T, E, n))
            cx, cv = rng.standard_normal((E, N)), rng.standard_normal((E, N))
            fwd, out = _taped(env, G, T, every, cot, cm, cx, cv)
            assert np.array_equal(out["modes"], fwd["modes"])
            gG = _gain_grad(out)
            S = ha.Setup(N, Ng, L, 1.0, env.dt)
            for e in range(E):
                wG, wx, wv, wm, wa = hf.autograd_vjp(x0[e], v0[e], G[e], S, T, M, cot[:, :, e], cm[:, e], cx[e], cv[e])
                assert _rel(fwd["modes"][:, e], wm) < 1e-9 and _rel(fwd["actions"][:, e], wa) < 1e-9
                errs = (_rel(gG[e], wG), _rel(out["g_x0"][e], wx), _rel(out["g_v0"][e], wv))
                worst = max(worst, *errs)
                assert max(errs) < PARITY_BOUND, (T, every, e, errs)
            env.close()
    record_measure(f"feedback_gain_grad_rel_err_E{E}_bpe{bpe}", worst)


def test_directional_derivative_in_gain_matches_central_differences():
    E, N, Ng, T = 2, 3000, 64, 8
    n = 2 * M
    rng = np.random.default_rng(5)
    G = np.stack([hf.g0(M) + 0.2 * rng.standard_normal((n, n)) for _ in range(E)])
    D = rng.standard_normal((E, n, n))
    w = rng.standard_normal((T, 3, E))

    def J(gain):
        env, _, _ = _make(E, N, Ng, seed=5)
        r = env.step_feedback_gain(gain, T, history=True)
        env.close()
        return (np.stack([r["KE"], r["PE"], r["PE_reward"]], 1) * w).sum()
    env, _, _ = _make(E, N, Ng, seed=5)
    _, out = _taped(env, G, T, 0, w)
    env.close()
    dd = float((_gain_grad(out) * D).sum())
    h = 1e-5
    fd = (J(G + h * D) - J(G - h * D)) / (2 * h)
    record_measure("feedback_gain_fd_rel_err", abs(dd - fd) / abs(fd))
    assert abs(dd - fd) < 1e-4 * abs(fd), (dd, fd)


def test_gradients_are_bitwise_reproducible():
    E, N, Ng, T = 3, 3000, 64, 7
    n = 2 * M
    rng = np.random.default_rng(2)
    G = np.stack([hf.g0(M) + 0.3 * rng.standard_normal((n, n)) for _ in range(E)])
    cot = rng.standard_normal((T, 3, E))
    cm = rng.standard_normal((T, E, n))
    cx, cv = rng.standard_normal((E, N)), rng.standard_normal((E, N))

    def run(every=0, **kw):
        env, _, _ = _make(E, N, Ng, seed=2, **kw)
        _, out = _taped(env, G, T, every, cot, cm, cx, cv)
        sched = env._h.schedule()
        env.close()
        return out, sched

    ref, s0 = run()
    assert s0 == "resident" and run(blocks_per_env=2)[1] == "streaming"
    variants = [run()[0], run(blocks_per_env=1)[0], run(blocks_per_env=2)[0], run(blocks_per_env=-1)[0]]
    variants += [run(every=k)[0] for k in (1, 3, T)]
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
    _, alone = _taped(one, G[1:2], T, 0, cot[:, :, 1:2], cm[:, 1:2], cx[1:2], cv[1:2])
    for k in ("g_ext", "g_actions", "modes"):
        assert np.array_equal(alone[k][:, 0], ref[k][:, 1]), k
    for k in ("g_x0", "g_v0"):
        assert np.array_equal(alone[k][0], ref[k][1]), k
    one.close()


@pytest.mark.parametrize("bpe", [0, 2])
def test_taping_does_not_change_the_forward(bpe):
    E, N, Ng, T = 2, 3000, 64, 9
    G = _random_gain(E, 2 * M, 3)
    taped, _, _ = _make(E, N, Ng, seed=4, blocks_per_env=bpe)
    twin, _, _ = _make(E, N, Ng, seed=4, blocks_per_env=bpe)
    taped.start_tape(T, 4)
    ra = taped.step_feedback_gain(G, T, actions=True, modes=True, history=True)
    rb = twin.step_feedback_gain(G, T, actions=True, modes=True, history=True)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert _same(_state(taped), _state(twin))
    taped.stop_tape()
    taped.close()
    twin.close()


@pytest.mark.parametrize("bpe", [0, 2])
def test_mixed_tape_matches_autograd(bpe):
    E, N, Ng = 2, 3000, 64
    n = 2 * M
    T1, T2, T3 = 3, 4, 2
    T = T1 + T2 + T3
    rng = np.random.default_rng(8)
    a1 = rng.uniform(-0.5, 0.5, (T1, E, n))
    a3 = rng.uniform(-0.5, 0.5, (T3, E, n))
    G = np.stack([hf.g0(M) + 0.3 * rng.standard_normal((n, n)) for _ in range(E)])
    cot = rng.standard_normal((T, 3, E))
    cx, cv = rng.standard_normal((E, N)), rng.standard_normal((E, N))
    env, _, _ = _make(E, N, Ng, seed=8, blocks_per_env=bpe)
    x0, v0 = [np.asarray(a).copy() for a in env.particles()]
    env.start_tape(T, 3)
    env.step_actions_traj(a1)
    env.step_feedback_gain(G, T2)
    env.step_actions_traj(a3)
    plain = env._h.tape_backward(cot, cx, cv, ext=True, actions=True, particles=True)
    out = env._h.tape_backward_feedback(cot, cx, cv, None)
    res = env.backward(d_KE=cot[:, 0], d_PE=cot[:, 1], d_PE_reward=cot[:, 2], d_x=cx, d_v=cv)
    st = env.tape_stats()
    env.stop_tape()
    env.close()
    assert st["replay_mismatches"] == 0
    for k in ("g_ext", "g_actions", "g_x0", "g_v0"):
        assert np.array_equal(plain[k], out[k]), k
    assert not out["modes"][:T1].any() and not out["modes"][T1 + T2:].any() and out["modes"][T1:T1 + T2].any()
    assert np.array_equal(res["gain"], _gain_grad(out, T1, T2))
    S = ha.Setup(N, Ng, L, 1.0, 0.1)
    import torch
    B = torch.as_tensor(hf.basis(L, Ng, M))
    Jm = torch.as_tensor(hf.jacobian(Ng, M))
    worst = 0.0
    for e in range(E):
        x = torch.as_tensor(x0[e]).clone().requires_grad_(True)
        v = torch.as_tensor(v0[e]).clone().requires_grad_(True)
        Gt = torch.as_tensor(G[e]).clone().requires_grad_(True)
        xs, vs, hist = x, v, []
        Ecur = ha.field(ha.density(xs, S), S)
        for t in range(T):
            act = torch.as_tensor(a1[t, e]) if t < T1 else (Gt @ (Jm @ Ecur) if t < T1 + T2 else torch.as_tensor(a3[t - T1 - T2, e]))
            xs, vs, ke, pe, per, Ecur = ha.step(xs, vs, B @ act, S)
            hist.append(torch.stack([ke, pe, per]))
        Jo = (torch.stack(hist) * torch.as_tensor(cot[:, :, e])).sum() + (xs * torch.as_tensor(cx[e])).sum() + (vs * torch.as_tensor(cv[e])).sum()
        wG, wx, wv = torch.autograd.grad(Jo, (Gt, x, v))
        errs = (_rel(res["gain"][e], wG.numpy()), _rel(out["g_x0"][e], wx.numpy()), _rel(out["g_v0"][e], wv.numpy()))
        worst = max(worst, *errs)
        assert max(errs) < PARITY_BOUND, (e, errs)
    record_measure(f"feedback_gain_mixed_rel_err_bpe{bpe}", worst)


def test_one_gradient_step_lowers_J():
    import torch
    from ocplasma_amd.env.grad import rollout_feedback
    E, N, Ng, T, lam = 3, 3000, 64, 10, 0.1
    G = torch.as_tensor(np.stack([hf.g0(M)] * E), device="cuda").requires_grad_(True)

    def J(gain, grad):
        env, _, _ = _make(E, N, Ng, seed=9)
        ke, pe, per, modes = rollout_feedback(env, gain, T)
        acts = torch.einsum("eik,tek->tei", gain, modes)
        j = per.sum(0) + lam * (acts ** 2).sum((0, 2)) * L / 4
        if grad:
            j.sum().backward()
        env.stop_tape()
        env.close()
        return j.detach().cpu().numpy()
    J0 = J(G, True)
    g = G.grad.detach()
    eta = 1e-3 * torch.as_tensor(J0, device="cuda") / (g ** 2).sum((1, 2))
    with torch.no_grad():
        J1 = J(G - eta[:, None, None] * g, False)
    assert np.all(J1 < J0), (J0, J1)


def test_refusals():
    from ocplasma_amd._abi import PicError
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    E, N, Ng = 1, 3000, 64
    env, _, _ = _make(E, N, Ng)
    G = np.stack([hf.g0(M)])
    with pytest.raises(PicError, match="max_mode"):
        r = env._h.lib.pic_step_feedback_gain(env._h._h, M + 1, G.ctypes.data, 0, 1, None, None, None)
        env._h._chk(r)
    env.start_tape(2)
    env.step_feedback_gain(G, 2)
    with pytest.raises(PicError, match="max_steps"):
        env.step_feedback_gain(G, 1)
    with pytest.raises(PicError, match="refused while a tape is open"):
        env.step_feedback(1)
    env.stop_tape()
    bare = BatchedPIC(1, N, Ng, L=L, dt=0.1)
    x, v = po.synthetic_bump_on_tail(N, L, seed=1)
    bare.reset(x[None], v[None])
    bare.max_mode = M
    bare._h.max_mode = M
    with pytest.raises(PicError, match="pic_set_actuator"):
        bare.step_feedback_gain(G, 1)
    env.close()
    bare.close()
