"""Closed loops under a torch policy on the device (pic_tape_walk_*, env.grad.rollout_policy): the walk against
the monolithic backward bit for bit, the linear policy against the gain law, policy gradients against torch autograd of the
restatement (tests/hp_policy.py) and against finite differences, bitwise reproducibility, and the walk's contract."""
import numpy as np
import pytest
import torch

import hp_feedback as hf
import hp_policy as hpp
from conftest import record_measure, rel_err
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
GRAD_BOUND = 4.4e-12          # 100 x the largest relative error measured against autograd, 4.4e-14 (policy_grad_rel_err_*)
LAW_BOUND = 3e-12             # test_gpu_feedback_gain.py's PARITY_BOUND


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


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- 1. the walk is the monolithic backward -----------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3, 0])
def test_walk_without_injections_is_tape_backward_bit_for_bit(every):
    E, N, Ng, T = 2, 3000, 64, 7
    env, X, V = _make(E, N, Ng, seed=2)
    rng = np.random.default_rng(every)
    acts = rng.uniform(-1, 1, (T, E, 2 * M))
    hist, cx, cv = rng.standard_normal((T, 3, E)), rng.standard_normal((E, N)), rng.standard_normal((E, N))
    env.start_tape(T, every)
    env.step_actions_traj(acts)
    want = env._h.tape_backward(hist, cx, cv, ext=True, actions=True, particles=True)
    for on_device in (False, True):
        w = env.walk(M, on_device=on_device)
        for t in range(T - 1, -1, -1):
            last = t == T - 1
            conv = (lambda a: torch.as_tensor(a, device="cuda")) if on_device else (lambda a: a)
            s, g_ext, g_act = w.step(d_energies=conv(hist[t]), d_x=conv(cx) if last else None, d_v=conv(cv) if last else None)
            assert s == t
            assert _same_bits(g_ext, want["g_ext"][t]) and _same_bits(g_act, want["g_actions"][t]), (on_device, t)
        g_x0, g_v0 = w.end()
        assert _same_bits(g_x0, want["g_x0"]) and _same_bits(g_v0, want["g_v0"]), on_device
    env.stop_tape()
    env.close()


@pytest.mark.parametrize("every", [1, 2, 0])
def test_walk_of_a_gain_law_tape_is_tape_backward_feedback_bit_for_bit(every):
    E, N, Ng, T = 2, 3000, 64, 6
    env, X, V = _make(E, N, Ng, seed=4)
    rng = np.random.default_rng(10 + every)
    G = hf.g0(M)[None] + rng.uniform(-0.3, 0.3, (E, 2 * M, 2 * M))
    hist, cm = rng.standard_normal((T, 3, E)), rng.standard_normal((T, E, 2 * M))
    env.start_tape(T, every)
    env.step_feedback_gain(G, T)
    for modes in (False, True):
        want = env._h.tape_backward_feedback(hist, None, None, cm if modes else None)
        w = env.walk(M)
        for t in range(T - 1, -1, -1):
            dm = cm[t + 1] if modes and t + 1 < T else None           # m_{t+1} is the modes of the field step t left
            s, g_ext, g_act = w.step(d_energies=hist[t], d_modes=dm)
            assert s == t and _same_bits(g_ext, want["g_ext"][t]) and _same_bits(g_act, want["g_actions"][t]), (modes, t)
        g_x0, g_v0 = w.end(d_modes0=cm[0] if modes else None)
        assert _same_bits(g_x0, want["g_x0"]) and _same_bits(g_v0, want["g_v0"]), modes
    env.stop_tape()
    env.close()


# ---- 2. the linear policy is the gain law ---------------------------------------------------------------------------------------
def test_linear_policy_on_modes_matches_rollout_feedback():
    from ocplasma_amd.env import grad
    E, N, Ng, T = 3, 4000, 64, 8
    G = torch.as_tensor(hf.g0(M) + np.random.default_rng(1).uniform(-0.2, 0.2, (2 * M, 2 * M)), device="cuda")
    out = {}
    for kind in ("law", "policy"):
        env, X, V = _make(E, N, Ng, seed=5)
        g = G.clone().requires_grad_(True)
        if kind == "law":
            ke, pe, per, modes = grad.rollout_feedback(env, g, T)
        else:
            ke, pe, per, acts, obs = grad.rollout_policy(env, lambda m: m @ g.T, T, observe="modes")
            modes = torch.stack(obs[:T])
        J = per.sum() + 0.1 * pe.sum() + 0.5 * (modes ** 2).sum()
        J.backward()
        out[kind] = [t.detach().cpu().numpy() for t in (ke, pe, per, modes, g.grad)]
        env.stop_tape()
        env.close()
    errs = [rel_err(a, b) for a, b in zip(out["policy"], out["law"])]
    record_measure("policy_grad_linear_vs_law_rel_err", max(errs))
    assert max(errs) < LAW_BOUND, errs


# ---- 3. policy gradients against autograd of the restatement ---------------------------------------------------------------
def _device_params(p):
    return {k: t.to("cuda").clone().requires_grad_(True) for k, t in p.items()}


def _policy(kind, p):
    return (lambda o: hpp.mlp_modes(p, o)) if kind == "modes" else (lambda o: hpp.deepsets_state(p, o, L))


def _params(kind, E, Mo, seed):
    lead = (E,) if E else ()
    if kind == "modes":
        return hpp.mlp_params(2 * Mo, 2 * M, 8, lead=lead, seed=seed)
    return hpp.deepsets_params(2 * M, 8, lead=lead, seed=seed)


def _weights(T, E, Mo, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, E, 3)), rng.standard_normal((E, 2 * Mo))


def _device_loss(env, kind, p, T, Mo, w_hist, w_obs, every=0):
    from ocplasma_amd.env import grad
    ke, pe, per, acts, obs = grad.rollout_policy(env, _policy(kind, p), T, observe=kind, obs_modes=Mo, checkpoint_every=every)
    wh = torch.as_tensor(w_hist, device="cuda")
    J = (torch.stack([ke, pe, per], -1) * wh).sum() + 0.05 * (acts ** 2).sum()
    if kind == "modes":
        J = J + (obs[-1] * torch.as_tensor(w_obs, device="cuda")).sum()
    return J, acts


@pytest.mark.parametrize("kind,E,N,T", [("modes", 2, 2000, 5), ("modes", 4, 5000, 20), ("state", 2, 2000, 5), ("state", 3, 5000, 12)])
def test_policy_gradients_match_autograd(kind, E, N, T):
    Ng, Mo = 64, 4
    env, X, V = _make(E, N, Ng, seed=7)
    env.use_torch_stream()
    p = _device_params(_params(kind, E, Mo, seed=3))
    w_hist, w_obs = _weights(T, E, Mo, seed=4)
    J, _ = _device_loss(env, kind, p, T, Mo, w_hist, w_obs)
    J.backward()
    S = hpp.ha.Setup(N, Ng, L, 1.0, 0.1)
    worst = 0.0
    for e in range(E):
        pe_ = {k: t.detach().cpu()[e].clone().requires_grad_(True) for k, t in p.items()}
        hist, acts, obs = hpp.rollout(torch.as_tensor(X[e]), torch.as_tensor(V[e]), _policy(kind, pe_), S, T, M, kind, Mo)
        Jc = hpp.loss_terms(hist, acts, obs, w_hist[:, e], 0.05, w_obs[e] if kind == "modes" else None)
        gc = torch.autograd.grad(Jc, list(pe_.values()))
        gd = np.concatenate([p[k].grad[e].cpu().numpy().ravel() for k in pe_])
        err = rel_err(gd, np.concatenate([g.numpy().ravel() for g in gc]))
        worst = max(worst, err)
    record_measure(f"policy_grad_rel_err_{kind}_E{E}_N{N}_T{T}", worst)
    assert worst < GRAD_BOUND, worst
    env.stop_tape()
    env.close()


# ---- 4. a directional derivative against device finite differences -----------------------------------------------------------
def test_directional_derivative_matches_device_finite_differences():
    E, N, Ng, T, Mo = 2, 5000, 64, 8, 4
    env, X, V = _make(E, N, Ng, seed=8)
    p = _device_params(_params("modes", E, Mo, seed=5))
    w_hist, w_obs = _weights(T, E, Mo, seed=6)
    J, _ = _device_loss(env, "modes", p, T, Mo, w_hist, w_obs)
    J.backward()
    rng = np.random.default_rng(11)
    eps, worst = 1e-6, 0.0
    for _ in range(3):
        d = {k: torch.as_tensor(rng.standard_normal(t.shape), device="cuda") for k, t in p.items()}
        an = float(sum((p[k].grad * d[k]).sum() for k in p))
        f = []
        for s in (eps, -eps):
            env.stop_tape()
            env.reset(X, V)
            with torch.no_grad():
                f.append(float(_device_loss(env, "modes", {k: t.detach() + s * d[k] for k, t in p.items()}, T, Mo, w_hist, w_obs)[0]))
        fd = (f[0] - f[1]) / (2 * eps)
        worst = max(worst, abs(fd - an) / abs(an))
    record_measure("policy_grad_fd_rel_eps1e-6", worst)
    assert worst < 1.3e-7, worst         # 100 x the 1.3e-9 measured at eps = 1e-6
    env.stop_tape()
    env.close()


# ---- 5. bitwise reproducibility -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["modes", "state"])
def test_policy_gradients_are_bitwise_independent_of_schedule_and_interval(kind):
    E, N, Ng, T, Mo = 2, 3000, 64, 7, 3
    w_hist, w_obs = _weights(T, E, Mo, seed=12)
    ref = None
    for bpe, every in ((0, 0), (2, 0), (0, 1), (3, 4), (0, 7)):
        env, X, V = _make(E, N, Ng, seed=9, blocks_per_env=bpe)
        p = _device_params(_params(kind, E, Mo, seed=13))
        J, _ = _device_loss(env, kind, p, T, Mo, w_hist, w_obs, every)
        J.backward()
        g = [_bits(p[k].grad) for k in sorted(p)]
        if ref is None:
            ref = g
        assert all(np.array_equal(a, b) for a, b in zip(g, ref)), (bpe, every)
        env.stop_tape()
        env.close()


# ---- 6. the walk's contract -----------------------------------------------------------------------------------------------------
def test_walk_contract():
    from ocplasma_amd._abi import PicError
    from ocplasma_amd.env import grad
    env, X, V = _make(2, 2000, 64, seed=10)
    with pytest.raises(PicError, match="-3"):
        env._h.tape_walk_begin(M)                                     # no tape
    env.start_tape(6, 2)
    env.step_actions_traj(np.zeros((4, 2, 2 * M)))
    for f in (lambda: env._h.tape_walk_step(0, 0, 0, 0, 0, 0, 0), lambda: env._h.tape_walk_end(0, 0, 0, 0, 0, 0)):
        with pytest.raises(PicError, match="no walk in progress"):
            f()
    with pytest.raises(PicError, match="-1"):
        env.walk(64)                                                  # obs_modes must be < N_mesh
    w = env.walk()
    assert w.step()[0] == 3
    with pytest.raises(PicError, match="not walked yet"):
        w.end()
    env.step_actions(np.zeros((2, 2 * M)))                            # appending abandons the walk
    with pytest.raises(PicError, match="no walk in progress"):
        w.step()
    w = env.walk()
    assert [w.step()[0] for _ in range(5)] == [4, 3, 2, 1, 0]
    with pytest.raises(PicError, match="every step has been walked"):
        w.step()
    w2 = env.walk()                                                   # a new walk replaces the first
    with pytest.raises(PicError):
        w.end()
    env._h.tape_backward(None)                                        # a backward abandons a walk too
    with pytest.raises(PicError, match="no walk in progress"):
        w2.step()
    env.stop_tape()
    # a rollout_policy whose environment moved on
    p = _device_params(_params("modes", 2, M, seed=1))
    ke, pe, per, acts, obs = grad.rollout_policy(env, _policy("modes", p), 3)
    env.stop_tape()
    env.reset(X, V)                                                   # (the tape holds exactly T steps: a reset moves on)
    with pytest.raises(PicError, match="moved on"):
        per.sum().backward()
    env.stop_tape()
    env.reset(X, V)
    ke, pe, per, acts, obs = grad.rollout_policy(env, _policy("modes", p), 3)
    grad.rollout_policy(env, _policy("modes", p), 2)                  # another rollout restarts the tape
    with pytest.raises(PicError, match="moved on"):
        per.sum().backward()
    env.stop_tape()
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    bare = BatchedPIC(1, 2000, 64, L=L, dt=0.1)
    bare.reset_sampled("two-stream")
    with pytest.raises(PicError, match="actuator"):
        grad.rollout_policy(bare, lambda m: m, 2)
    bare.close()
    env.close()
    del oc


# ---- 7. one gradient step on the example's policy ----------------------------------------------------------------------------
def test_one_gradient_step_lowers_the_cost_in_every_environment():
    from ocplasma_amd.env import grad
    E, N, Ng, T, Mo, lam = 4, 5000, 250, 12, 5, 0.1

    def cost(p, env):
        ke, pe, per, acts, obs = grad.rollout_policy(env, _policy("modes", p), T, obs_modes=Mo)
        return per.sum(0) + lam * (acts ** 2).sum((0, 2)) * L / 4         # the reference's cost, per environment
    env, X, V = _make(E, N, Ng, seed=11, M_=M)
    env.use_torch_stream()
    p = _device_params(_params("modes", E, Mo, seed=7))
    J0 = cost(p, env)
    J0.sum().backward()
    sq = sum((t.grad ** 2).flatten(1).sum(1) for t in p.values())
    eta = 1e-3 * J0.detach() / sq
    with torch.no_grad():
        q = {k: t - eta.view(-1, *([1] * (t.dim() - 1))) * t.grad for k, t in p.items()}
        env.stop_tape()
        env.reset(X, V)
        J1 = cost(q, env)
    assert bool(torch.all(J1 < J0.detach())), (J0, J1)
    env.stop_tape()
    env.close()
