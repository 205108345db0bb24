"""The per-step smoothed KL on the tape (pic_tape_kl_*): the trace against kl_smooth of an untaped twin and the
restatement, the forward untouched, the gradient against autograd of the restatement (tests/hp_tape_kl.py), bitwise
determinism, the walk, the C contract and the torch entries.

Default shapes: 2 environments of N = 3001 (odd: a half-filled 16-byte tile, and ld = 3008 != N) on 64 nodes, T = 5 steps with
checkpoint intervals 1, 2 and 0 (= 3: the last segment is partial); N = 3001 runs the resident schedule by default and the
streaming one with blocks_per_env = 2; N = 20000 spreads an environment's deposit over three workgroups."""
import numpy as np
import pytest
import torch

import hp_adjoint as ha
import hp_phase as hp
import hp_tape_kl as hk
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
VMIN, VMAX = -6.0, 6.0
TOL_KL = 3.4e-14              # test_gpu_phase_kl.py's bound for the same quantity
# 100 x the largest relative-norm error measured on an MI355X against autograd of the restatement, 4.5e-14 (g_actions at
# N = 20000; keys "tape_kl.grad.*", profiles/tape_kl.md); its ingredients: 1.3e-13 for the adjoint, 5.4e-16 for the KL's
# gradient.  Ceiling: 1e-9 (test_gpu_adjoint.py: PARITY_BOUND).
GRAD_BOUND = 4.5e-12
E0, N0, NG0, T0 = 2, 3001, 64, 5


def _make(E=E0, N=N0, Ng=NG0, seed=1, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    X, V = np.empty((E, N)), np.empty((E, N))
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


def _feq(E, nx, nv, per_env, seed, vmin=VMIN, vmax=VMAX):
    shape = (E, nx, nv) if per_env else (nx, nv)
    return np.random.default_rng(seed).uniform(0.0, 2.0 / (L * (vmax - vmin)), shape)


def _kl(feq, vmin=VMIN, vmax=VMAX):
    return dict(feq=feq, vmin=vmin, vmax=vmax)


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _healthy(env):
    st = env.tape_stats()
    assert st["replay_mismatches"] == 0 and st["unit_retries"] == 0 and st["replay_bad_positions"] == 0, st
    return st


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("ext", "actions", "x0", "v0"))


# ---- 1. the trace ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nx,nv,per_env,vr,every", [(N0, 32, 32, False, (VMIN, VMAX), 2), (N0, 64, 1024, True, (-2.0, 3.0), 1),
                                                      (20000, 32, 32, True, (VMIN, VMAX), 0)])
def test_trace_is_kl_smooth_after_every_step(N, nx, nv, per_env, vr, every):
    a = _actions(T0, E0, 1)
    feq = _feq(E0, nx, nv, per_env, 2, *vr)
    env, X, V = _make(N=N)
    if vr[1] < VMAX:
        assert np.any(V > vr[1]) and np.any(V < vr[0])                # dropped particles occur
    env.start_tape(T0, every, kl=_kl(feq, *vr))
    env.step_actions_traj(a)
    trace = env.tape_kl()
    assert trace.shape == (T0, E0)
    assert np.array_equal(env.tape_kl(on_device=True).cpu().numpy(), trace)
    env.backward(d_KL=np.ones((T0, E0)))
    _healthy(env)
    env.stop_tape()
    env.close()
    twin, _, _ = _make(N=N)
    G = hp.Grid(nx, nv, L, vr[0], vr[1], N, twin.n0)
    worst = 0.0
    for t in range(T0):
        twin.step_actions_traj(a[t:t + 1])
        assert np.array_equal(trace[t], twin.kl_smooth(feq, *vr)), t
        x, v = (torch.as_tensor(p) for p in twin.particles())
        ref = hp.kl(hp.density(x, v, G), torch.as_tensor(feq), G).numpy()
        worst = max(worst, float(np.max(np.abs(trace[t] - ref)) / np.max(np.abs(ref))))
    record_measure(f"tape_kl.trace.N{N}_{nx}x{nv}", worst)
    assert worst <= TOL_KL
    twin.close()


# ---- 2. the forward is untouched ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,sched", [({}, "resident"), ({"blocks_per_env": 2}, "streaming")])
@pytest.mark.parametrize("entry", ["actions", "ext", "gain"])
def test_forward_is_bitwise_that_of_a_plain_tape(kw, sched, entry):
    a = _actions(T0, E0, 3)
    feq = _feq(E0, 32, 32, False, 4)
    gain = 0.05 * np.random.default_rng(5).standard_normal((E0, 2 * M, 2 * M))
    outs = []
    for kl in (None, _kl(feq)):
        env, _, _ = _make(**kw)
        assert env._h.schedule() == sched
        env.start_tape(T0, 2, kl=kl)
        if entry == "actions":
            tr = env.step_actions_traj(a, history=True)
        elif entry == "ext":
            tr = env.step_ext_traj(_ext_of(a, NG0), history=True)
        else:
            o = env.step_feedback_gain(gain, T0, modes=True, history=True)
            tr = (o["KE"], o["PE"], o["PE_reward"], o["modes"])
        outs.append(list(env.particles()) + [env.fields()[1]] + list(tr))
        if kl is not None:
            assert np.all(np.isfinite(env.tape_kl()))
        env.stop_tape()
        env.close()
    for p, q in zip(*outs):
        assert np.array_equal(p, q)


# ---- 3. the gradient against autograd of the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("N,nx,nv,per_env,vr,every", [(N0, 32, 32, False, (VMIN, VMAX), 2), (N0, 64, 1024, True, (-2.0, 3.0), 1),
                                                      (20000, 32, 32, False, (VMIN, VMAX), 0)])
def test_gradient_matches_autograd_of_the_restatement(N, nx, nv, per_env, vr, every):
    rng = np.random.default_rng(N + nx)
    a = _actions(T0, E0, 6)
    feq = _feq(E0, nx, nv, per_env, 7, *vr)
    d_kl, cot = rng.standard_normal((T0, E0)), rng.standard_normal((T0, 3, E0))
    cx, cv = rng.standard_normal((E0, N)), rng.standard_normal((E0, N))
    env, _, _ = _make(N=N, seed=3)
    x0, v0 = env.particles()
    env.start_tape(T0, every, kl=_kl(feq, *vr))
    env.step_actions_traj(a)
    out = env.backward(d_KE=cot[:, 0], d_PE=cot[:, 1], d_PE_reward=cot[:, 2], d_x=cx, d_v=cv, d_KL=d_kl)
    _healthy(env)
    env.stop_tape()
    S = ha.Setup(N, NG0, L, 1.0, env.dt)
    G = hp.Grid(nx, nv, L, vr[0], vr[1], N, env.n0)
    ext = _ext_of(a, NG0)
    worst = 0.0
    for e in range(E0):
        fe = feq[e] if per_env else feq
        ge, gx, gv = hk.autograd_vjp(x0[e], v0[e], ext[:, e], S, G, fe, d_kl[:, e], cot[:, :, e], cx[e], cv[e])
        errs = (_rel(out["ext"][:, e], ge), _rel(out["actions"][:, e], _bt(ge, NG0)), _rel(out["x0"][e], gx), _rel(out["v0"][e], gv))
        worst = max(worst, *errs)
    record_measure(f"tape_kl.grad.N{N}_{nx}x{nv}", worst)
    assert worst < GRAD_BOUND, worst
    env.close()


# ---- 4. the KL alone equals the existing route ------------------------------------------------------------------------------------
def test_kl_of_the_last_step_equals_kl_smooth_grad_into_a_plain_backward():
    a = _actions(T0, E0, 8)
    feq = _feq(E0, 32, 32, True, 9)
    d = np.array([0.7, -1.3])
    d_kl = np.zeros((T0, E0))
    d_kl[-1] = d
    env, _, _ = _make()
    env.start_tape(T0, 2, kl=_kl(feq))
    env.step_actions_traj(a)
    new = env.backward(d_KL=d_kl)
    _healthy(env)
    env.stop_tape()
    env.close()
    env, _, _ = _make()
    env.start_tape(T0, 2)
    env.step_actions_traj(a)
    gx, gv = env.kl_smooth_grad(feq, d, VMIN, VMAX)
    old = env.backward(d_x=gx, d_v=gv)
    _healthy(env)
    env.stop_tape()
    env.close()
    assert _same(new, old)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------
def test_gradients_with_kl_cotangents_are_bitwise_reproducible():
    rng = np.random.default_rng(10)
    a = _actions(T0, E0, 10)
    feq = _feq(E0, 64, 1024, False, 11)
    d_kl, cot = rng.standard_normal((T0, E0)), rng.standard_normal((T0, 3, E0))

    def run(every=0, envs=slice(None), **kw):
        E = len(range(E0)[envs])
        env, X, V = _make(**kw)
        if E != E0:
            env.close()
            from ocplasma_amd.env.batched import BatchedPIC
            import ocplasma_amd as oc
            env = BatchedPIC(E, N0, NG0, L=L, dt=0.1, **kw)
            env.reset(X[envs], V[envs])
            env.set_actuator(oc.E_field(L, NG0, M))
        env.start_tape(T0, every, kl=_kl(feq))
        env.step_actions_traj(a[:, envs])
        out = env.backward(d_KE=cot[:, 0, envs], d_PE=cot[:, 1, envs], d_PE_reward=cot[:, 2, envs], d_KL=d_kl[:, envs])
        out["kl"] = env.tape_kl()
        _healthy(env)
        sched = env._h.schedule()
        env.stop_tape()
        env.close()
        return out, sched

    ref, s0 = run()
    assert s0 == "resident"
    for kw in (dict(blocks_per_env=1), dict(blocks_per_env=2), dict(blocks_per_env=-1), dict(every=1), dict(every=2)):
        got, sched = run(**kw)
        assert _same(got, ref) and np.array_equal(got["kl"], ref["kl"]), kw
        if kw.get("blocks_per_env") == 2:
            assert sched == "streaming"
    alone, _ = run(envs=slice(1, 2))
    assert np.array_equal(alone["kl"][:, 0], ref["kl"][:, 1])
    for k in ("ext", "actions"):
        assert np.array_equal(alone[k][:, 0], ref[k][:, 1]), k
    assert np.array_equal(alone["x0"][0], ref["x0"][1]) and np.array_equal(alone["v0"][0], ref["v0"][1])


# ---- 6. no cotangent, no change ----------------------------------------------------------------------------------------------------
def test_without_kl_cotangents_the_backward_is_a_plain_tapes():
    rng = np.random.default_rng(12)
    a = _actions(T0, E0, 12)
    feq = _feq(E0, 32, 32, False, 13)
    cot = rng.standard_normal((T0, 3, E0))
    cx, cv = rng.standard_normal((E0, N0)), rng.standard_normal((E0, N0))
    kw = dict(d_KE=cot[:, 0], d_PE=cot[:, 1], d_PE_reward=cot[:, 2], d_x=cx, d_v=cv)
    env, _, _ = _make()
    env.start_tape(T0, 2)
    env.step_actions_traj(a)
    plain = env.backward(**kw)
    base = _healthy(env)["launches"]
    env.stop_tape()
    env.close()
    env, _, _ = _make()
    env.start_tape(T0, 2, kl=_kl(feq))
    env.step_actions_traj(a)
    assert _same(env.backward(**kw), plain)
    assert _healthy(env)["launches"] == base
    with_kl = env.backward(d_KL=np.ones((T0, E0)), **kw)
    assert _healthy(env)["launches"] == base + 3 * T0
    assert not np.array_equal(with_kl["x0"], plain["x0"])
    assert _same(env.backward(**kw), plain)                          # d_KL = None clears the rows again
    assert _healthy(env)["launches"] == base
    rows = np.ones((2, E0))
    from ocplasma_amd._abi import PIC_HOST
    env._h.tape_kl_cot(rows.ctypes.data, PIC_HOST, 1, 2)             # k = 2 steps flagged
    hist = np.ascontiguousarray(cot)
    env._h.tape_backward(hist, cx, cv, ext=True, actions=True, particles=True)
    assert _healthy(env)["launches"] == base + 3 * 2
    env.stop_tape()
    env.close()


# ---- 7. the walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 2, 0])
def test_walk_with_kl_cotangents_equals_the_backward(every):
    rng = np.random.default_rng(14)
    a = _actions(T0, E0, 14)
    feq = _feq(E0, 32, 32, True, 15)
    d_kl, cot = rng.standard_normal((T0, E0)), rng.standard_normal((T0, 3, E0))
    cx, cv = rng.standard_normal((E0, N0)), rng.standard_normal((E0, N0))
    env, _, _ = _make()
    env.start_tape(T0, every, kl=_kl(feq))
    env.step_actions_traj(a)
    want = env.backward(d_KE=cot[:, 0], d_PE=cot[:, 1], d_PE_reward=cot[:, 2], d_x=cx, d_v=cv, d_KL=d_kl)
    for on_device in (False, True):
        conv = (lambda p: torch.as_tensor(p, device="cuda")) if on_device else (lambda p: p)
        host = (lambda p: p.cpu().numpy()) if on_device else (lambda p: p)
        w = env.walk(M, on_device=on_device)
        for t in range(T0 - 1, -1, -1):
            last = t == T0 - 1
            s, g_ext, g_act = w.step(d_energies=conv(cot[t]), d_x=conv(cx) if last else None, d_v=conv(cv) if last else None,
                                     d_kl=conv(d_kl[t]))
            assert s == t and np.array_equal(host(g_ext), want["ext"][t]) and np.array_equal(host(g_act), want["actions"][t])
        g_x0, g_v0 = w.end()
        assert np.array_equal(host(g_x0), want["x0"]) and np.array_equal(host(g_v0), want["v0"]), on_device
        _healthy(env)
    env.stop_tape()
    env.close()


# ---- 8. the contract -----------------------------------------------------------------------------------------------------------------
def _r256(n):
    return (n + 255) // 256 * 256


def test_contract():
    from ocplasma_amd._abi import PIC_HOST, PicError
    a = _actions(T0, E0, 16)
    nx, nv = 24, 40
    feq = _feq(E0, nx, nv, False, 17)
    env, X, V = _make()
    h = env._h

    def start(f=feq, nx_=nx, nv_=nv, lo=VMIN, hi=VMAX):
        h.tape_kl_start(nx_, nv_, lo, hi, f.ctypes.data if f is not None else 0, 0, PIC_HOST)
    buf = np.zeros((T0, E0))
    with pytest.raises(PicError, match="-3"):
        start()                                                       # no tape
    env.start_tape(T0, 2)
    plain_bytes = env.tape_stats()["bytes"]
    for bad in (dict(nx_=0), dict(nv_=1025), dict(lo=1.0, hi=1.0), dict(f=None)):
        with pytest.raises(PicError, match="-1"):
            start(**bad)
    for f in (lambda: h.tape_kl(PIC_HOST, buf.ctypes.data), lambda: h.tape_kl_cot(buf.ctypes.data, PIC_HOST, 0, 0),
              lambda: env.tape_kl()):
        with pytest.raises(PicError):
            f()                                                       # no KL on this tape
    with pytest.raises(ValueError, match="d_KL"):
        env.backward(d_KL=buf)
    env.stop_tape()
    env.start_tape(T0, 2, kl=_kl(feq))
    with pytest.raises(PicError, match="-3"):
        start()                                                       # a KL already
    nb = nx * nv
    want = _r256(8 * nb) + 2 * _r256(8 * E0 * nb) + 2 * _r256(8 * T0 * E0)
    assert env.tape_stats()["bytes"] == plain_bytes + want
    env.step_actions_traj(a[:3])
    assert env.tape_kl().shape == (3, E0)
    for first, n in ((-1, 1), (0, 4), (3, 1), (2, 2), (0, -1)):
        with pytest.raises(PicError, match="-1"):
            h.tape_kl_cot(buf.ctypes.data, PIC_HOST, first, n)
    with pytest.raises(PicError, match="-1"):
        h.tape_kl_cot(buf.ctypes.data, 7, 0, 1)                       # bad mem_kind
    h.tape_kl_cot(buf.ctypes.data, PIC_HOST, 3, 0)                    # an empty range at the end is fine
    # during a walk: rows of steps already reversed are refused, the others are taken and the walk goes on
    w = env.walk()
    h.tape_kl_cot(np.ones((3, E0)).ctypes.data, PIC_HOST, 0, 3)
    assert w.step(d_kl=np.ones(E0))[0] == 2
    with pytest.raises(PicError, match="-3"):
        h.tape_kl_cot(buf.ctypes.data, PIC_HOST, 2, 1)
    with pytest.raises(PicError, match="-3"):
        h.tape_kl_cot(None, PIC_HOST, 0, 3)
    h.tape_kl_cot(buf.ctypes.data, PIC_HOST, 0, 2)
    assert [w.step()[0] for _ in range(2)] == [1, 0]
    w.end()
    _healthy(env)
    env.step_actions_traj(a[3:])
    with pytest.raises(PicError, match="-3"):
        start()                                                       # the tape holds steps
    # tangent ignores the KL
    d_act = np.random.default_rng(18).standard_normal((T0, E0, 2 * M))
    tan = env.tangent(d_actions=d_act)
    grad_kl = env.backward(d_PE_reward=np.ones((T0, E0)))
    env.stop_tape()
    # stop, then a plain tape: as ever
    env.reset(X, V)
    env.start_tape(T0, 2)
    env.step_actions_traj(a)
    with pytest.raises(PicError):
        env.tape_kl()
    tan_plain = env.tangent(d_actions=d_act)
    grad_plain = env.backward(d_PE_reward=np.ones((T0, E0)))
    assert all(np.array_equal(tan[k], tan_plain[k]) for k in tan)
    assert _same(grad_kl, grad_plain)
    env.stop_tape()
    # one byte short of what the KL needs: PIC_ENOMEM, and the tape works without one
    env.reset(X, V)
    with pytest.raises(PicError, match="-4"):
        env.start_tape(T0, 2, budget_bytes=plain_bytes + want - 1, kl=_kl(feq))
    assert env.tape_stats()["bytes"] == plain_bytes
    env.step_actions_traj(a)
    assert _same(env.backward(d_PE_reward=np.ones((T0, E0))), grad_plain)
    _healthy(env)
    env.stop_tape()
    env.reset(X, V)
    env.start_tape(T0, 2, budget_bytes=plain_bytes + want, kl=_kl(feq))    # exactly enough
    env.stop_tape()
    env.close()


# ---- 9. torch ----------------------------------------------------------------------------------------------------------------------
def test_torch_rollouts_return_and_differentiate_the_kl():
    from ocplasma_amd.env import grad
    a = _actions(T0, E0, 19)
    feq = _feq(E0, 32, 32, False, 20)
    env, X, V = _make()
    at = torch.tensor(a, device="cuda", requires_grad=True)
    outs = grad.rollout(env, at, kl=_kl(feq))
    assert len(outs) == 4
    ke, pe, per, kl = outs
    trace = env.tape_kl()
    assert np.array_equal(kl.detach().cpu().numpy(), trace)
    (g,) = torch.autograd.grad(kl.sum() + per.sum(), at)
    want = env.backward(d_PE_reward=np.ones((T0, E0)), d_KL=np.ones((T0, E0)))["actions"]
    assert np.array_equal(g.cpu().numpy(), want)
    _healthy(env)
    env.stop_tape()
    env.reset(X, V)
    et = torch.tensor(_ext_of(a, NG0), requires_grad=True)            # host tensors, raw fields
    _, _, _, kl_e = grad.rollout_ext(env, et, kl=_kl(feq))
    assert np.array_equal(kl_e.detach().numpy(), trace)
    (ge,) = torch.autograd.grad(kl_e.sum(), et)
    assert np.array_equal(ge.numpy(), env.backward(d_KL=np.ones((T0, E0)))["ext"])
    env.stop_tape()
    env.reset(X, V)
    assert len(grad.rollout(env, at)) == 3                            # without kl: today's arity
    env.stop_tape()
    env.reset(X, V)
    gt = torch.tensor(0.05 * np.random.default_rng(21).standard_normal((2 * M, 2 * M)), device="cuda", requires_grad=True)
    outs = grad.rollout_feedback(env, gt, T0, kl=_kl(feq))
    assert len(outs) == 5 and outs[4].shape == (T0, E0)
    (gg,) = torch.autograd.grad(outs[4].sum(), gt)
    assert bool(torch.isfinite(gg).all()) and float(gg.abs().max()) > 0
    _healthy(env)
    env.stop_tape()
    env.close()


def test_rollout_policy_with_kl_equals_a_manual_walk():
    from ocplasma_amd.env import grad
    T, Mo = 3, 2
    feq = _feq(E0, 32, 32, False, 22)
    env, X, V = _make()
    env.use_torch_stream()
    gen = torch.Generator().manual_seed(1)
    p = [(0.3 * torch.randn(s, generator=gen, dtype=torch.float64)).cuda().requires_grad_(True) for s in ((2 * Mo, 8), (8, 2 * M))]
    policy = lambda o: torch.tanh(o @ p[0]) @ p[1]                    # noqa: E731
    for it in range(2):
        env.stop_tape()
        env.reset(X, V)
        ke, pe, per, acts, obs, kl = grad.rollout_policy(env, policy, T, obs_modes=Mo, kl=_kl(feq))
        assert kl.shape == (T, E0) and np.array_equal(kl.detach().cpu().numpy(), env.tape_kl())
        got = torch.autograd.grad(kl.sum() + per.sum(), p)
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in got)
        # the same by hand: reverse step t, then the policy's own vector-Jacobian product between two reverse steps
        want = [torch.zeros_like(q) for q in p]
        w = env.walk(Mo, on_device=True)
        d_en = torch.zeros((3, E0), dtype=torch.float64, device="cuda")
        d_en[2] = 1.0
        g_obs = None
        for t in range(T - 1, -1, -1):
            _, _, g_act = w.step(d_energies=d_en, d_modes=g_obs, d_kl=torch.ones(E0, dtype=torch.float64, device="cuda"))
            o = obs[t].detach().requires_grad_(True)
            gs = torch.autograd.grad(policy(o), p + [o], g_act)
            want = [x + y for x, y in zip(want, gs[:2])]
            g_obs = gs[2]
        w.end(d_modes0=g_obs)
        _healthy(env)
        for x, y in zip(got, want):
            assert _rel(x.cpu().numpy(), y.cpu().numpy()) < 1e-14     # (the sums over t run in another order)
        with torch.no_grad():
            for q, g in zip(p, got):
                q -= 1e-3 * g
    env.stop_tape()
    env.close()
