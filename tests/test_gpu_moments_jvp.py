"""Forward mode of the fluid moments on the device (pic_moments_jvp, pic_tape_moments_start / pic_tape_moments,
pic_tape_tangent_moments): the stand-alone tangents against a longdouble evaluation of the equations on the
device's own particles, direction groups on grid z, refusals, non-finite input, duality with pic_moments_vjp, bitwise
guarantees, the trace on the tape, the tape's tangents against torch forward-mode AD and against backward(d_moments=), and the
torch entries."""
import numpy as np
import pytest
import torch

import hp_adjoint as ha
import hp_moments as hm
import hp_moments_jvp as hj
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
LD = hj.LD
# Asserted bounds: 100 x the largest value measured on an MI355X (recorded as moments_jvp.*), with a ceiling of 1e-9.  Every
# comparison is a relative norm per (direction, environment, moment) against the restatement (longdouble for one state, torch
# forward-mode AD or autograd for rollouts), never against another output of the device.  The stand-alone error grows with N
# because the unit leaves 61 - b bits under the largest term of a moment (2^b >= N) and the terms of dm2 have long tails
# (|iota| v^2): at N = 20000 a term is rounded to 2^-46 of the largest, against node sums of about 160 terms that cancel.
ALONE_BOUND = 1.9e-11         # measured 1.85e-13 at (2, 20000, 250) after 5 steps (1.79e-13 after the reset; 2.4e-14 at N = 3000; 2.4e-16 hand-placed)
GROUPS_BOUND = 1.2e-12        # measured 1.11e-14 (Ng = 512, K = 8); 7.9e-15 (Ng = 2722, K = 2)
DUAL_BOUND = 7.8e-12          # measured 7.71e-14 at (2, 20000, 250); 6.3e-14 at (2, 3000, 64)
INVARIANT_BOUND = 1.4e-12     # measured 1.32e-14 at (2, 20000, 250); 1.7e-15 at (2, 3000, 64)
TAPE_BOUND = 1.5e-11          # measured 1.41e-13 at (2, 20000, 250, T = 5); 1.1e-14 at (2, 3000, 64, T = 5); 7.8e-15 at T = 1
TAPE_DUAL_BOUND = 7.5e-11     # measured 7.48e-13 at (2, 20000, 250, T = 5); 8.3e-14 and 1.5e-14 at N = 3000
TORCH_BOUND = 6.2e-13         # measured 6.16e-15 at (2, 3000, 64, T = 4), both modes


def _sample(E, N, seed=1):
    X = np.empty((E, N))
    V = np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=seed + 7 * e)
    return X, V


def _make(E, N, Ng, seed=1, actuator=False, XV=None, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    X, V = _sample(E, N, seed) if XV is None else XV
    env.reset(X, V)
    if actuator:
        env.set_actuator(oc.E_field(L, Ng, M))
    return env, X, V


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _directions(K, E, N, seed):
    """K random directions; direction 2 (if any) is all zero."""
    rng = np.random.default_rng(seed)
    dx, dv = rng.standard_normal((K, E, N)), rng.standard_normal((K, E, N))
    if K > 2:
        dx[2] = dv[2] = 0.0
    return dx, dv


def _reference(env, dx, dv):
    """[K, E, 3, Ng] longdouble on the particles the device holds (dx, dv: [K, E, N] or None)."""
    x, v = env.particles()
    K = (dx if dx is not None else dv).shape[0]
    ref = np.zeros((K, env.num_envs, 3, env.N_mesh), dtype=LD)
    for k in range(K):
        for e in range(env.num_envs):
            ref[k, e] = hj.jvp_ld(x[e], v[e], None if dx is None else dx[k, e], None if dv is None else dv[k, e], env.N_mesh, L,
                                  env.n0)
    return ref


def _worst(got, ref):
    """max over (direction, environment, moment) of the relative-norm error; a zero reference row must be +0 bit for bit."""
    worst = 0.0
    got = np.asarray(got)
    for idx in np.ndindex(ref.shape[:-1]):
        r = ref[idx]
        if not r.any():
            assert not _bits(got[idx]).any(), idx
            continue
        worst = max(worst, float(np.linalg.norm((got[idx].astype(LD) - r).astype(np.float64)) / np.linalg.norm(r.astype(np.float64))))
    return worst


# ---- 1. stand-alone against longdouble --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,Ng,steps", [(2, 3000, 64, 0), (2, 2999, 64, 0), (1, 1, 16, 0), (3, 65, 16, 0), (2, 20000, 250, 0),
                                          (2, 20000, 250, 5)])
def test_jvp_matches_the_longdouble_restatement(E, N, Ng, steps):
    X, V = _sample(E, N, seed=3)
    if E > 1:
        V[1] = 0.0                                        # an environment at rest: dm2 = +0 there
    env, _, _ = _make(E, N, Ng, XV=(X, V))
    if steps:
        env.step(nsteps=steps)
    dx, dv = _directions(8, E, N, seed=N + Ng)
    ref = _reference(env, dx, dv)
    worst = 0.0
    full = env.moments_jvp(dx, dv)
    assert full.shape == (8, E, 3, Ng)
    for K in (1, 4, 5, 8):
        got = env.moments_jvp(dx[:K], dv[:K])
        assert _same(got, full[:K]), K                    # K directions in one call are the first K of 8
        worst = max(worst, _worst(got, ref[:K]))
    assert not _bits(full[2]).any()                       # the all-zero direction: +0 on every node
    if E > 1 and not steps:
        assert not _bits(full[:, 1, 2]).any()             # v = 0: dm2 = 2 w v dv - iota v^2 = +0
    # one direction without the leading axis; d_x alone and d_v alone (NULL for the other)
    assert _same(env.moments_jvp(dx[0], dv[0]), full[0])
    only_x, only_v = env.moments_jvp(d_x=dx[:4]), env.moments_jvp(d_v=dv[:4])
    worst = max(worst, _worst(only_x, _reference(env, dx[:4], None)), _worst(only_v, _reference(env, None, dv[:4])))
    assert not _bits(only_v[:, :, 0]).any()               # no position tangent: dm0 = +0
    assert _same(only_x, env.moments_jvp(dx[:4], np.zeros_like(dv[:4])))
    # device memory gives the same bits
    dev = env.moments_jvp(torch.as_tensor(dx, device="cuda"), torch.as_tensor(dv, device="cuda"))
    assert dev.is_cuda and _same(dev, full)
    assert env.bad_count() == 0
    env.close()
    name = f"moments_jvp.alone.E{E}_N{N}_Ng{Ng}_s{steps}"
    print(f"{name} = {worst:.3e}")
    record_measure(name, worst)
    assert worst < ALONE_BOUND, worst


def test_hand_placed_particles_at_the_edges():
    """Particles exactly at x = 0 and in the last cell, whose right node is node 0."""
    Ng = 8
    dxm = L / Ng
    x = np.array([0.0, 3 * dxm, np.nextafter(L, 0.0), L - 0.25 * dxm, 20.3, 33.3])
    v = np.array([1.5, -2.0, 0.7, 0.0, 3.0, -1.0])
    env, _, _ = _make(2, 6, Ng, XV=(np.stack([x, x]), np.stack([v, v[::-1].copy()])))
    dx, dv = _directions(2, 2, 6, seed=4)
    got = env.moments_jvp(dx, dv)
    worst = _worst(got, _reference(env, dx, dv))
    # the particle in the last cell moves mass between node Ng - 1 and node 0
    only = np.zeros((2, 6))
    only[:, 3] = 1.0
    m = env.moments_jvp(d_x=only)
    assert m[0, 0, 0] > 0 and m[0, 0, Ng - 1] < 0 and not m[0, 0, 1:Ng - 1].any()
    env.close()
    print(f"moments_jvp.alone.hand_placed = {worst:.3e}")
    record_measure("moments_jvp.alone.hand_placed", worst)
    assert worst < ALONE_BOUND, worst


# ---- 2. direction groups ---------------------------------------------------------------------------------------------------------
# Three LDS meshes of Ng + 1 words per direction in 64 KB: 5 directions at Ng = 512 (8 directions: groups of 5 and 3 on grid z),
# one from Ng = 1365 on.  A float64 handle itself exists up to Ng = 2722 (pic_create: the sweeps' own LDS meshes), so that is
# the largest mesh the one-direction groups can be run at; the entry's own limit of 2728 cells lies above it.
@pytest.mark.parametrize("Ng,K", [(512, 8), (2722, 2)])
def test_direction_groups_on_grid_z(Ng, K):
    E, N = 2, 3001
    env, _, _ = _make(E, N, Ng, seed=5)
    dx, dv = _directions(K, E, N, seed=Ng)
    got = env.moments_jvp(dx, dv)
    worst = _worst(got, _reference(env, dx, dv))
    for k in range(K):
        assert _same(env.moments_jvp(dx[k], dv[k]), got[k]), k
    env.close()
    print(f"moments_jvp.groups.Ng{Ng}_K{K} = {worst:.3e}")
    record_measure(f"moments_jvp.groups.Ng{Ng}_K{K}", worst)
    assert worst < GROUPS_BOUND, worst


def test_a_mesh_too_large_is_refused():
    from ocplasma_amd._abi import PicError
    from ocplasma_amd.env.batched import BatchedPIC
    with pytest.raises(PicError, match=r"\(-1\)|error -1"):
        env = BatchedPIC(1, 1000, 2729, L=L, dt=0.1)      # (no float64 handle has 2729 cells: pic_create's own limit comes first)
        X, V = _sample(1, 1000)
        env.reset(X, V)
        env.moments_jvp(d_x=np.ones((1, 1000)))


# ---- 3. other refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,why", [(dict(dtype="float32"), "float64"), (dict(dtype="float32", position_dtype="fixed32"), "float64"),
                                    (dict(interpol="TSC"), "TSC")])
def test_jvp_refuses_what_is_not_differentiated(kw, why):
    from ocplasma_amd._abi import PicError
    env, X, V = _make(2, 1000, 32, **kw)
    with pytest.raises(PicError, match="error -1.*" + why):
        env.moments_jvp(d_x=np.ones((2, 1000)))
    env.close()


def test_jvp_refuses_bad_direction_counts_and_a_handle_without_state():
    from ocplasma_amd._abi import PIC_HOST, PicError
    from ocplasma_amd.env.batched import BatchedPIC
    E, N, Ng = 2, 1000, 32
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    out = np.zeros((9, E, 3, Ng))
    d = np.ones((9, E, N))
    with pytest.raises(PicError, match="error -3"):       # before reset
        env._h.moments_jvp(1, d.ctypes.data, 0, PIC_HOST, out.ctypes.data)
    env.reset(*_sample(E, N))
    for K in (0, 9):
        with pytest.raises(PicError, match="error -1.*1 <= K <= 8"):
            env._h.moments_jvp(K, d.ctypes.data, 0, PIC_HOST, out.ctypes.data)
    with pytest.raises(ValueError, match="directions"):
        env.moments_jvp(d[:2], d[:3])
    env.close()


# ---- 4. non-finite input ---------------------------------------------------------------------------------------------------------
def test_a_non_finite_tangent_marks_its_direction_and_environment_alone():
    E, N, Ng, K = 3, 3001, 64, 4
    env, _, _ = _make(E, N, Ng, seed=6)
    dx, dv = _directions(K, E, N, seed=8)
    clean = env.moments_jvp(dx, dv)
    bad = dv.copy()
    bad[1, 2, 7] = np.inf
    got = env.moments_jvp(dx, bad)
    assert np.isnan(got[1, 2, 1:]).all()                  # dm1 and dm2 of that (direction, environment)
    assert _same(got[1, 2, 0], clean[1, 2, 0])            # dm0 does not see dv
    keep = np.ones((K, E), dtype=bool)
    keep[1, 2] = False
    assert _same(got[keep], clean[keep])
    assert _same(env.moments_jvp(dx, dv), clean)          # the accumulators were cleared behind the NaN
    env.close()


# ---- 5. duality and invariants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,Ng", [(2, 3000, 64), (2, 20000, 250)])
def test_duality_with_the_vjp_and_the_invariants(E, N, Ng):
    env, _, _ = _make(E, N, Ng, seed=9)
    env.step(nsteps=2)
    x, v = env.particles()
    dx, dv = _directions(2, E, N, seed=10)
    c = np.random.default_rng(11).standard_normal((E, 3, Ng))
    jm = env.moments_jvp(dx, dv)
    S = ha.Setup(N, Ng, L, 1.0, env.dt)
    dual = inv = 0.0
    for e in range(E):
        gx, gv = hm.autograd_vjp(x[e], v[e], c[e], S)     # the restatement's gather, not the device's
        for k in range(2):
            lhs = float((c[e].astype(LD) * jm[k, e].astype(LD)).sum())
            rhs = float((gx.astype(LD) * dx[k, e]).sum() + (gv.astype(LD) * dv[k, e]).sum())
            dual = max(dual, abs(lhs - rhs) / abs(rhs))
            # sum_j dm0_j = 0 exactly in integers; in doubles up to the rounding of Ng conversions
            inv = max(inv, abs(float(jm[k, e, 0].astype(LD).sum())) / float(np.abs(jm[k, e, 0]).sum()))
            # sum_j dm2_j N dx / (2 n0 L) = sum_i v_i dv_i
            want = float((v[e].astype(LD) * dv[k, e].astype(LD)).sum())
            have = float(jm[k, e, 2].astype(LD).sum() * (LD(N) * (LD(L) / LD(Ng)) / (2 * LD(env.n0) * LD(L))))
            inv = max(inv, abs(have - want) / float(np.abs(v[e] * dv[k, e]).sum()))
    env.close()
    print(f"moments_jvp.dual.E{E}_N{N}_Ng{Ng} = {dual:.3e}   moments_jvp.invariants = {inv:.3e}")
    record_measure(f"moments_jvp.dual.E{E}_N{N}_Ng{Ng}", dual)
    record_measure(f"moments_jvp.invariants.E{E}_N{N}_Ng{Ng}", inv)
    assert dual < DUAL_BOUND, dual
    assert inv < INVARIANT_BOUND, inv


# ---- 6. bitwise ------------------------------------------------------------------------------------------------------------------
def test_jvp_is_bitwise_reproducible_and_perturbs_nothing():
    E, N, Ng, K = 6, 3001, 64, 4
    env, X, V = _make(E, N, Ng, seed=12)
    env.step(nsteps=2)
    x, v = env.particles()
    dx, dv = _directions(K, E, N, seed=13)
    m0, g0 = env.moments(), env.moments_vjp(np.ones((E, 3, Ng)))
    want = env.moments_jvp(dx, dv)
    assert _same(env.moments_jvp(dx, dv), want)
    for k in range(K):                                    # K directions in one call equal K calls
        assert _same(env.moments_jvp(dx[k], dv[k]), want[k]), k
    # pic_moments and pic_moments_vjp keep their bits with calls interleaved
    assert _same(env.moments(), m0)
    g1 = env.moments_vjp(np.ones((E, 3, Ng)))
    assert _same(g1[0], g0[0]) and _same(g1[1], g0[1])
    env.close()
    for blocks in (0, 2, 7):
        other, _, _ = _make(E, N, Ng, XV=(x, v), blocks_per_env=blocks)
        assert _same(other.moments_jvp(dx, dv), want), blocks
        other.close()
    alone, _, _ = _make(1, N, Ng, XV=(x[3:4], v[3:4]))    # an environment alone and in a batch of 6
    assert _same(alone.moments_jvp(dx[:, 3:4], dv[:, 3:4])[:, 0], want[:, 3])
    alone.close()
    # the steps and the fields keep their bits with calls interleaved
    out = []
    for look in (True, False):
        env, _, _ = _make(E, N, Ng, XV=(X, V))
        env.step(nsteps=2)
        if look:
            env.moments_jvp(dx, dv)
        env.step(nsteps=2)
        out.append((*env.particles(), *env.fields(), *env.energies()))
        env.close()
    for a, b in zip(*out):
        assert _same(a, b)


# ---- 7. the trace on the tape ----------------------------------------------------------------------------------------------------
T7 = 5


def _actions(T, E, seed=12):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (T, E, 2 * M))


@pytest.mark.parametrize("blocks,schedule", [(0, "resident"), (2, "streaming")])
def test_trace_rows_are_the_moments_of_every_step(blocks, schedule):
    E, N, Ng = 2, 3000, 64
    a = _actions(T7, E)
    dper = np.random.default_rng(3).standard_normal((T7, E))
    env, X, V = _make(E, N, Ng, seed=11, actuator=True, blocks_per_env=blocks)
    assert env._h.schedule() == schedule
    env.start_tape(T7, 2, moments=True)
    ke, pe, per = env.step_actions_traj(a, history=True)
    trace = env.tape_moments()
    assert trace.shape == (T7, E, 3, Ng)
    assert _same(env.tape_moments(on_device=True), trace)
    grads = env.backward(d_PE_reward=dper)
    state = env.particles()
    env.stop_tape()
    env.close()
    # a twin stepped one call at a time, with pic_moments after every step
    twin, _, _ = _make(E, N, Ng, XV=(X, V), actuator=True, blocks_per_env=blocks)
    for t in range(T7):
        twin.step_actions(a[t])
        assert _same(twin.moments(), trace[t]), t
    twin.close()
    # the same tape without the trace: particles, energies and gradients keep their bits
    plain, _, _ = _make(E, N, Ng, XV=(X, V), actuator=True, blocks_per_env=blocks)
    plain.start_tape(T7, 2)
    ke0, pe0, per0 = plain.step_actions_traj(a, history=True)
    g0 = plain.backward(d_PE_reward=dper)
    for got, want in zip((ke, pe, per, *state), (ke0, pe0, per0, *plain.particles())):
        assert _same(got, want)
    for k in g0:
        assert _same(grads[k], g0[k]), k
    plain.stop_tape()
    plain.close()


def test_trace_contract():
    from ocplasma_amd._abi import PicError
    E, N, Ng = 2, 3000, 64
    a = _actions(T7, E)
    env, X, V = _make(E, N, Ng, seed=11, actuator=True)
    with pytest.raises(PicError, match="error -3"):       # no tape
        env._h.tape_moments_start()
    env.start_tape(T7, 2)
    plain = env.tape_stats()["bytes"]
    env.step_actions_traj(a[:1])
    with pytest.raises(PicError, match="error -3"):       # a start after a step
        env._h.tape_moments_start()
    with pytest.raises(PicError, match="tape_moments"):
        env.tape_moments()
    env.stop_tape()
    env.reset(X, V)
    want = (8 * T7 * E * 3 * Ng + 255) // 256 * 256       # [max_steps][env][3][Ng] float64, rounded up to 256 bytes
    env.start_tape(T7, 2, moments=True)
    assert env.tape_stats()["bytes"] == plain + want
    with pytest.raises(PicError, match="error -3"):       # a second start
        env._h.tape_moments_start()
    assert env.tape_moments().shape == (0, E, 3, Ng)
    env.stop_tape()
    with pytest.raises(PicError, match="error -4"):       # one byte short: the tape stays open without a trace
        env.start_tape(T7, 2, budget_bytes=plain + want - 1, moments=True)
    assert env.tape_stats()["bytes"] == plain
    env.step_actions_traj(a)
    assert np.isfinite(env.backward(d_PE_reward=np.ones((T7, E)))["actions"]).all()
    env.stop_tape()
    env.start_tape(T7, 2, budget_bytes=plain + want, moments=True)      # exactly enough
    env.step_actions_traj(a)
    assert np.isfinite(env.tape_moments()).all()
    env.stop_tape()
    env.close()


# ---- 8. the tape's tangents -------------------------------------------------------------------------------------------------------
def _ext_of(actions, Ng):
    T, E, _ = actions.shape
    out = np.empty((T, E, Ng))
    for t in range(T):
        for e in range(E):
            out[t, e] = po.actuator_field(L, Ng, M, actions[t, e, :M], actions[t, e, M:]).ravel()
    return out


def _tape_inputs(E, N, T, K, seed):
    rng = np.random.default_rng(seed)
    return dict(d_actions=rng.standard_normal((K, T, E, 2 * M)), d_x0=0.1 * rng.standard_normal((K, E, N)),
                d_v0=0.1 * rng.standard_normal((K, E, N)))


@pytest.mark.parametrize("E,N,Ng,T", [(2, 3000, 64, 1), (2, 3000, 64, 5), (2, 20000, 250, 5)])
def test_tape_tangents_match_forward_ad_and_are_dual_to_the_backward(E, N, Ng, T):
    K = 2
    a = _actions(T, E, seed=14)
    ins = _tape_inputs(E, N, T, K, seed=15)
    env, X, V = _make(E, N, Ng, seed=16, actuator=True)
    env.start_tape(T, 2)                                  # no trace needed: only the replayed states
    env.step_actions_traj(a)
    plain = env.tangent(**ins)
    base = env.tape_stats()["launches"]
    nseg = (T + 1) // 2
    assert base == 1 + 11 * T + 8 * T + nseg              # the start kernel, 11 per step, and the replay's
    got = env.tangent(moments=True, **ins)
    st = env.tape_stats()
    assert st["launches"] == base + 3 * T and st["replay_mismatches"] == 0, st
    assert got["moments"].shape == (K, T, E, 3, Ng)
    for k in plain:                                       # every other key keeps its bits
        assert _same(got[k], plain[k]), k
    dev = env.tangent(moments=True, **{k: torch.as_tensor(v, device="cuda") for k, v in ins.items()})
    assert _same(dev["moments"], got["moments"])
    # torch forward-mode AD of the restatement
    S = ha.Setup(N, Ng, L, 1.0, env.dt)
    ext = _ext_of(a, Ng)
    worst = 0.0
    for k in range(K):
        dext = _ext_of(ins["d_actions"][k], Ng)           # (the actuator is linear)
        for e in range(E):
            want = hj.rollout_torch_jvp(X[e], V[e], ext[:, e], S, d_ext=dext[:, e], d_x0=ins["d_x0"][k, e], d_v0=ins["d_v0"][k, e])
            for t in range(T):
                for m in range(3):
                    worst = max(worst, _rel(got["moments"][k, t, e, m], want[t, m]))
    # duality with backward(d_moments=c) under zero energy cotangents, against the restatement's gradient
    c = np.random.default_rng(17).standard_normal((T, E, 3, Ng))
    dual = 0.0
    for e in range(E):
        x0 = torch.as_tensor(X[e]).clone().requires_grad_(True)
        v0 = torch.as_tensor(V[e]).clone().requires_grad_(True)
        et = torch.as_tensor(ext[:, e]).clone().requires_grad_(True)
        mom = hm.rollout_moments(x0, v0, et, S)[3]
        ge, gx, gv = (t_.numpy() for t_ in torch.autograd.grad((mom * torch.as_tensor(c[:, e])).sum(), (et, x0, v0)))
        for k in range(K):
            dext = _ext_of(ins["d_actions"][k], Ng)
            rhs = float((ge * dext[:, e]).sum() + (gx * ins["d_x0"][k, e]).sum() + (gv * ins["d_v0"][k, e]).sum())
            lhs = float((c[:, e] * got["moments"][k, :, e]).sum())
            dual = max(dual, abs(lhs - rhs) / abs(rhs))
    # and the device's own pair: sum c . dm = <g_actions, u> + <g_x0, dx0> + <g_v0, dv0>, to the same bound
    res = env.backward(d_moments=c)
    for k in range(K):
        lhs = float((c * got["moments"][k]).sum())
        rhs = float((res["actions"] * ins["d_actions"][k]).sum() + (res["x0"] * ins["d_x0"][k]).sum() + (res["v0"] * ins["d_v0"][k]).sum())
        dual = max(dual, abs(lhs - rhs) / abs(rhs))
    env.stop_tape()
    env.close()
    print(f"moments_jvp.tape.E{E}_N{N}_Ng{Ng}_T{T} = {worst:.3e}   dual = {dual:.3e}")
    record_measure(f"moments_jvp.tape.E{E}_N{N}_Ng{Ng}_T{T}", worst)
    record_measure(f"moments_jvp.tape_dual.E{E}_N{N}_Ng{Ng}_T{T}", dual)
    assert worst < TAPE_BOUND, worst
    assert dual < TAPE_DUAL_BOUND, dual


def test_tape_tangents_are_independent_of_the_checkpoints_K_and_the_schedule():
    E, N, Ng, T, K = 2, 3000, 64, 5, 4
    a = _actions(T, E, seed=18)
    ins = _tape_inputs(E, N, T, K, seed=19)
    X, V = _sample(E, N, seed=20)
    want = None
    for kw, every in (({}, 2), ({}, 1), ({}, T), ({"blocks_per_env": 2}, 2)):
        env, _, _ = _make(E, N, Ng, XV=(X, V), actuator=True, **kw)
        assert env._h.schedule() == ("streaming" if kw else "resident")
        env.start_tape(T, every)
        env.step_actions_traj(a)
        got = env.tangent(moments=True, **ins)["moments"]
        if want is None:
            want = got
            for k in range(K):                            # K directions in one call equal K calls
                one = env.tangent(moments=True, **{n: v[k] for n, v in ins.items()})["moments"]
                assert one.shape == (T, E, 3, Ng) and _same(one, want[k]), k
        assert _same(got, want), (kw, every)
        env.stop_tape()
        env.close()


def test_tape_tangents_with_a_kl_as_well():
    E, N, Ng, T, K = 2, 3000, 64, 3, 2
    a = _actions(T, E, seed=21)
    ins = _tape_inputs(E, N, T, K, seed=22)
    env, X, V = _make(E, N, Ng, seed=23, actuator=True)
    feq = env.phase_density_smooth(32, -8.0, 8.0)[0] + 1e-3
    env.start_tape(T, 2, kl=dict(feq=feq, vmin=-8.0, vmax=8.0), moments=True)
    env.step_actions_traj(a)
    both = env.tangent(kl=True, moments=True, **ins)
    n_both = env.tape_stats()["launches"]
    kl = env.tangent(kl=True, **ins)
    n_kl = env.tape_stats()["launches"]
    mom = env.tangent(moments=True, **ins)
    assert n_both == n_kl + 3 * T
    assert set(both) == set(kl) | {"moments"} == set(mom) | {"KL"}
    for k in kl:
        assert _same(both[k], kl[k]), k
    for k in mom:
        assert _same(both[k], mom[k]), k
    # the trace is there too, and reading it changes nothing
    assert env.tape_moments().shape == (T, E, 3, Ng)
    env.stop_tape()
    env.close()


def test_a_gain_law_tape_stays_refused():
    from ocplasma_amd._abi import PicError
    E, N, Ng, T = 2, 3000, 64, 2
    env, X, V = _make(E, N, Ng, seed=24, actuator=True)
    env.start_tape(T, 2)
    env.step_feedback_gain(np.zeros((E, 2 * M, 2 * M)), T)
    with pytest.raises(PicError, match="gain law"):
        env.tangent(moments=True, d_x0=np.ones((E, N)))
    env.stop_tape()
    env.close()


# ---- 9. torch --------------------------------------------------------------------------------------------------------------------
def test_torch_rollout_with_moments_in_both_modes():
    import torch.autograd.forward_ad as fwAD
    from ocplasma_amd.env import grad
    E, N, Ng, T = 2, 3000, 64, 4
    a = _actions(T, E, seed=25)
    du = np.random.default_rng(26).standard_normal((T, E, 2 * M))
    target = 1.0 + 0.1 * np.cos(2 * np.pi * np.arange(Ng) / Ng)
    env, X, V = _make(E, N, Ng, seed=27, actuator=True)
    # defaults: three tensors with today's bits
    at = torch.as_tensor(a, device="cuda").requires_grad_(True)
    three = grad.rollout(env, at)
    assert len(three) == 3
    env.stop_tape()
    env.reset(X, V)
    hist = env.step_actions_traj(a, history=True)
    for got, want in zip(three, hist):
        assert _same(got, want)
    # moments=True: a fourth output, the trace
    env.reset(X, V)
    at = torch.as_tensor(a, device="cuda").requires_grad_(True)
    out = grad.rollout(env, at, moments=True)
    assert len(out) == 4 and tuple(out[3].shape) == (T, E, 3, Ng)
    assert _same(out[3], env.tape_moments())
    for got, want in zip(out[:3], three):
        assert _same(got, want)
    tt = torch.as_tensor(target, device="cuda")
    ((out[3][:, :, 0] - tt) ** 2).sum().backward()
    # autograd of the restatement
    S = ha.Setup(N, Ng, L, 1.0, env.dt)
    ext = _ext_of(a, Ng)
    bc, bs = po.actuator_basis(L, Ng, M)
    worst = 0.0
    for e in range(E):
        et = torch.as_tensor(ext[:, e]).clone().requires_grad_(True)
        mom = hm.rollout_moments(torch.as_tensor(X[e]), torch.as_tensor(V[e]), et, S)[3]
        (ge,) = torch.autograd.grad(((mom[:, 0] - torch.as_tensor(target)) ** 2).sum(), et)
        ge = ge.numpy()
        worst = max(worst, _rel(at.grad[:, e].cpu().numpy(), np.concatenate([ge @ bc, ge @ bs], axis=-1)))
    # forward mode, from the same start: the tangent of the trace equals tangent(moments=True)'s, and forward AD of the restatement
    env.stop_tape()
    env.reset(X, V)
    with fwAD.dual_level():
        dual = grad.rollout(env, fwAD.make_dual(torch.as_tensor(a, device="cuda"), torch.as_tensor(du, device="cuda")), moments=True)
        assert _same(fwAD.unpack_dual(dual[3]).primal, out[3])
        tan = fwAD.unpack_dual(dual[3]).tangent
        assert _same(tan, env.tangent(moments=True, d_actions=du)["moments"])
        tan = tan.cpu().numpy()
    dext = _ext_of(du, Ng)
    for e in range(E):
        want = hj.rollout_torch_jvp(X[e], V[e], ext[:, e], S, d_ext=dext[:, e])
        for t in range(T):
            for m in range(3):
                worst = max(worst, _rel(tan[t, e, m], want[t, m]))
    # with a KL as well: KE, PE, PE_reward, KL, moments
    env.stop_tape()
    env.reset(X, V)
    feq = env.phase_density_smooth(32, -8.0, 8.0)[0] + 1e-3
    five = grad.rollout(env, torch.as_tensor(a, device="cuda"), kl=dict(feq=feq, vmin=-8.0, vmax=8.0), moments=True)
    assert len(five) == 5 and tuple(five[3].shape) == (T, E) and tuple(five[4].shape) == (T, E, 3, Ng)
    assert _same(five[3], env.tape_kl()) and _same(five[4], out[3])
    env.stop_tape()
    env.close()
    print(f"moments_jvp.torch.E{E}_N{N}_Ng{Ng}_T{T} = {worst:.3e}")
    record_measure(f"moments_jvp.torch.E{E}_N{N}_Ng{Ng}_T{T}", worst)
    assert worst < TORCH_BOUND, worst
