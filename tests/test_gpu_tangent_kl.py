"""Forward mode of the smoothed KL on the device (pic_phase_kl_smooth_jvp, pic_tape_tangent_kl): the stand-alone
product against the device's own gradient, the tape's "KL" tangents against torch forward-mode AD of the restatement
(tests/hp_tangent_kl.py), duality with the device's adjoint, finite differences of the device's KL trace, bitwise invariants,
everything else untouched, the C contract and torch forward AD.

Shapes: 2 environments of N = 3001 (odd: a half-filled 16-byte tile, ld = 3008 != N, and dense rows that start on 8 bytes only;
resident by default, streaming with blocks_per_env = 2) or N = 20000 (three reduction chunks of 8192 particles, the last one
partial) on 64 nodes, T = 5 steps with checkpoint intervals 1, 2 and 0 (= 3: the last segment is partial); grids 32 x 32 with
a shared target and 96 x 96 with a target per environment (two LDS bands of the deposit); velocity ranges +-6 and +-2 (dropped
particles and clamped half-bins); K = 1, 3 and 8 directions."""
import numpy as np
import pytest
import torch

import hp_adjoint as ha
import hp_phase as hp
import hp_tangent_kl as htk
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
M = 3
E0, N0, N1, NG0, T0 = 2, 3001, 20000, 64, 5
WIDE, NARROW = (-6.0, 6.0), (-2.0, 2.0)
KL_LAUNCHES = 4               # kernels per step of the KL's tangent (include/picstep.h: pic_tape_tangent_kl)
CHUNK_TILES = 4096            # 16-byte tiles per reduction chunk (pic_phase.h: kJvpChunkTiles)
# Each bound is 100 x the largest relative-norm error measured on an MI355X against its own reference (keys "tangent_kl.*",
# profiles/tangent_kl.md); the factor covers other summation groupings at other shapes.
JVP_BOUND = 5.5e-14           # against the device's gradient dotted in longdouble: 5.50e-16 measured (N = 3001, 32 x 32, one side alone)
PARITY_BOUND = 5.3e-12        # against torch forward mode of the restatement: 5.26e-14 measured (N = 3001, 96 x 96, +-2); ceiling 1e-9
DUALITY_BOUND = 1.9e-11       # against the device's adjoint: 1.90e-13 measured (N = 20000, 32 x 32, +-2); ceiling 1e-10
FD_BOUND = 0.2                # against central differences of the device's KL trace at eps = 1e-6: 1.94e-3 measured (see the test)
FD_BOUND_1E4 = 1.2e-2         # the same at eps = 1e-4, where the rounding floor is 100 x lower: 1.17e-4 measured


def _make(E=E0, N=N0, Ng=NG0, seed=1, X=None, V=None, **kw):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    if X is None:
        X, V = np.empty((E, N)), np.empty((E, N))
        for e in range(E):
            X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=seed + 7 * e)
    env.reset(X, V)
    env.set_actuator(oc.E_field(L, Ng, M))
    return env, X, V


def _actions(T, E, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (T, E, 2 * M))


def _ext_of(actions, Ng):
    lead = actions.shape[:-1]
    flat = actions.reshape(-1, 2 * M)
    out = np.stack([po.actuator_field(L, Ng, M, a[:M], a[M:]).ravel() for a in flat])
    return out.reshape(lead + (Ng,))


def _feq(E, nx, nv, per_env, seed, vr):
    shape = (E, nx, nv) if per_env else (nx, nv)
    return np.random.default_rng(seed).uniform(0.0, 2.0 / (L * (vr[1] - vr[0])), shape)


def _kl(feq, vr):
    return dict(feq=feq, vmin=vr[0], vmax=vr[1])


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _healthy(env):
    st = env.tape_stats()
    assert st["replay_mismatches"] == 0 and st["unit_retries"] == 0 and st["replay_bad_positions"] == 0, st
    return st


def _drops_and_clamps(V, vr, nv):
    half = 0.5 * (vr[1] - vr[0]) / nv
    return (np.any(V > vr[1]) and np.any(V < vr[0]) and np.any((V >= vr[0]) & (V < vr[0] + half))
            and np.any((V <= vr[1]) & (V > vr[1] - half)))


def _r256(n):
    return (n + 255) // 256 * 256


def _kl_part_bytes(E, N):
    """include/picstep.h, pic_tape_tangent_kl: the unit cotangents and the chunks' sums of 8 directions."""
    chunks = -(-((N + 1) // 2) // CHUNK_TILES)
    return _r256(8 * E) + _r256(8 * 8 * E * chunks)


GRIDS = {"32s": (32, 32, False), "96e": (96, 96, True)}


# ---- 1. the stand-alone product ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,grid,vr,K", [(N0, "32s", WIDE, 1), (N0, "96e", NARROW, 3), (N1, "32s", NARROW, 8), (N1, "96e", WIDE, 3)])
def test_kl_smooth_jvp_is_the_devices_gradient_dotted_with_the_directions(N, grid, vr, K):
    nx, nv, per_env = GRIDS[grid]
    rng = np.random.default_rng(N + K)
    env, X, V = _make(N=N)
    if vr == NARROW:
        assert _drops_and_clamps(V, vr, nv)
    env.step_actions_traj(_actions(2, E0, 1))                            # (off the initial state: the wrapped x of a step)
    feq = _feq(E0, nx, nv, per_env, 2, vr)
    dx, dv = rng.standard_normal((K, E0, N)), rng.standard_normal((K, E0, N))
    gx, gv = env.kl_smooth_grad(feq, None, *vr)
    got = env.kl_smooth_jvp(feq, *vr, d_x=dx, d_v=dv)
    assert got.shape == (K, E0)
    ld = np.longdouble
    want = ((gx.astype(ld)[None] * dx.astype(ld)).sum(-1) + (gv.astype(ld)[None] * dv.astype(ld)).sum(-1)).astype(np.float64)
    err = _rel(got, want)
    # one side alone, no K axis, device memory: the same sums
    only_x = env.kl_smooth_jvp(feq, *vr, d_x=dx)
    only_v = env.kl_smooth_jvp(feq, *vr, d_v=dv)
    want_x = (gx.astype(ld)[None] * dx.astype(ld)).sum(-1).astype(np.float64)
    want_v = (gv.astype(ld)[None] * dv.astype(ld)).sum(-1).astype(np.float64)
    err = max(err, _rel(only_x, want_x), _rel(only_v, want_v))
    print(f"tangent_kl.jvp.N{N}_{grid}_K{K}: {err:.3e}")
    record_measure(f"tangent_kl.jvp.N{N}_{grid}_K{K}", err)
    one = env.kl_smooth_jvp(feq, *vr, d_x=dx[0], d_v=dv[0])
    assert one.shape == (E0,) and np.array_equal(one, got[0])
    dev = env.kl_smooth_jvp(torch.as_tensor(feq, device="cuda"), *vr, d_x=torch.as_tensor(dx, device="cuda"),
                            d_v=torch.as_tensor(dv, device="cuda"))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    assert np.array_equal(env.kl_smooth_jvp(feq, *vr, d_x=dx, d_v=dv), got)             # twice: the same bits
    assert np.array_equal(env.kl_smooth_jvp(feq, *vr), np.zeros(E0))                    # no tangent: 0
    assert err < JVP_BOUND, err
    env.close()


# ---- 2. parity with torch forward mode of the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("N,grid,vr,every,kw", [(N0, "32s", WIDE, 2, {}), (N0, "96e", NARROW, 1, {}),
                                                (N0, "96e", NARROW, 0, {"blocks_per_env": 2}), (N1, "32s", WIDE, 0, {})])
def test_kl_tangents_match_torch_forward_mode(N, grid, vr, every, kw):
    nx, nv, per_env = GRIDS[grid]
    rng = np.random.default_rng(N + every)
    a = _actions(T0, E0, 3)
    feq = _feq(E0, nx, nv, per_env, 4, vr)
    env, X, V = _make(N=N, seed=2, **kw)
    if N == N0:
        assert env._h.schedule() == ("streaming" if kw else "resident")
    x0, v0 = env.particles()
    da, dx0, dv0 = rng.standard_normal((T0, E0, 2 * M)), rng.standard_normal((E0, N)), rng.standard_normal((E0, N))
    env.start_tape(T0, every, kl=_kl(feq, vr))
    env.step_actions_traj(a)
    # three directions in one call: the actions alone, x0 alone, v0 alone
    out = env.tangent(d_actions=np.stack([da, 0 * da, 0 * da]), d_x0=np.stack([0 * dx0, dx0, 0 * dx0]),
                      d_v0=np.stack([0 * dv0, 0 * dv0, dv0]), kl=True)
    assert out["KL"].shape == (3, T0, E0)
    _healthy(env)
    env.stop_tape()
    S = ha.Setup(N, NG0, L, 1.0, env.dt)
    G = hp.Grid(nx, nv, L, vr[0], vr[1], N, env.n0)
    ext, dea = _ext_of(a, NG0), _ext_of(da, NG0)
    worst = 0.0
    for e in range(E0):
        fe = feq[e] if per_env else feq
        for k, u in enumerate((dict(d_ext=dea[:, e]), dict(d_x0=dx0[e]), dict(d_v0=dv0[e]))):
            _, tkl, _, _ = htk.torch_jvp(x0[e], v0[e], ext[:, e], S, G, fe, **u)
            assert np.any(tkl != 0.0)
            worst = max(worst, _rel(out["KL"][k][:, e], tkl))
    name = f"tangent_kl.parity.N{N}_{grid}_every{every}" + ("_streaming" if kw else "")
    print(f"{name}: {worst:.3e}")
    record_measure(name, worst)
    assert worst < PARITY_BOUND, worst
    env.close()


# ---- 3. duality with the device's adjoint --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,grid,vr,every", [(N0, "96e", NARROW, 1), (N0, "32s", WIDE, 2), (N1, "32s", NARROW, 0)])
def test_kl_tangents_are_dual_to_the_device_adjoint(N, grid, vr, every):
    """<k-bar, dKL> + <a-bar, dhist> from tangent(kl=True) = <g_actions, da> + <g_x0, dx0> + <g_v0, dv0> from backward(d_KL = k-bar)."""
    nx, nv, per_env = GRIDS[grid]
    rng = np.random.default_rng(N + every + 1)
    feq = _feq(E0, nx, nv, per_env, 6, vr)
    env, X, V = _make(N=N, seed=4)
    env.start_tape(T0, every, kl=_kl(feq, vr))
    env.step_actions_traj(_actions(T0, E0, 5))
    da, dx0, dv0 = rng.standard_normal((T0, E0, 2 * M)), rng.standard_normal((E0, N)), rng.standard_normal((E0, N))
    kbar, abar = rng.standard_normal((T0, E0)), rng.standard_normal((T0, 3, E0))
    out = env.tangent(d_actions=da, d_x0=dx0, d_v0=dv0, kl=True)
    g = env.backward(d_KE=abar[:, 0], d_PE=abar[:, 1], d_PE_reward=abar[:, 2], d_KL=kbar)
    gk = env.backward(d_KL=kbar)                                         # and the KL alone
    _healthy(env)
    env.stop_tape()
    worst = 0.0
    for e in range(E0):
        lk = float((kbar[:, e] * out["KL"][:, e]).sum())
        lhs = lk + float(sum((abar[:, i, e] * out[k][:, e]).sum() for i, k in enumerate(("KE", "PE", "PE_reward"))))
        for left, gg in ((lhs, g), (lk, gk)):
            rhs = float((gg["actions"][:, e] * da[:, e]).sum() + (gg["x0"][e] * dx0[e]).sum() + (gg["v0"][e] * dv0[e]).sum())
            worst = max(worst, abs(left - rhs) / max(abs(left), abs(rhs)))
    print(f"tangent_kl.duality.N{N}_{grid}_every{every}: {worst:.3e}")
    record_measure(f"tangent_kl.duality.N{N}_{grid}_every{every}", worst)
    assert worst < DUALITY_BOUND, worst
    env.close()


# ---- 4. finite differences of the device's own KL trace ----------------------------------------------------------------------------
def test_kl_directional_derivative_matches_device_finite_differences():
    """The target is the smoothed density of the starting state (the use of examples/kl_control.py): its cotangent grid is
    smooth, so the derivative adds up over the particles while the rounding of the integer weights (2^-25 of a particle per
    axis at N = 3001, which the difference quotient divides by eps) does not.  That rounding is the floor of this check: the
    relative-norm error of the [T, E] derivatives is 1.94e-3 on an MI355X, five orders above the parity with forward-mode AD, so
    the bound only catches a wrong sign, factor or step index.  (The derivatives of the steps nearly cancel in their sum over
    t, whose difference quotient is off by 2.7e-2: the trace is compared, not its sum.)  A second quotient at eps = 1e-4 lowers
    that floor a hundredfold and gives the case its discriminating power."""
    vr = WIDE
    env, X, V = _make(seed=5)
    a = _actions(T0, E0, 7)
    da = np.random.default_rng(8).standard_normal((T0, E0, 2 * M))
    feq = env.phase_density_smooth((32, 32), *vr)
    env.start_tape(T0, kl=_kl(feq, vr))
    env.step_actions_traj(a)
    an = env.tangent(d_actions=da, kl=True)["KL"]
    env.stop_tape()
    for eps, bound in ((1e-6, FD_BOUND), (1e-4, FD_BOUND_1E4)):
        trace = []
        for sgn in (1.0, -1.0):
            env.reset(X, V)
            env.start_tape(T0, kl=_kl(feq, vr))
            env.step_actions_traj(a + sgn * eps * da)
            trace.append(env.tape_kl())
            env.stop_tape()
        fd = (trace[0] - trace[1]) / (2 * eps)                          # [T, E]
        worst = _rel(an, fd)
        print(f"tangent_kl.fd_rel_eps{eps:g}: {worst:.3e}")
        record_measure(f"tangent_kl.fd_rel_eps{eps:g}", worst)
        assert worst < bound, (eps, worst)
    env.close()


# ---- 5. bitwise invariants -----------------------------------------------------------------------------------------------------
def _directions(K, N, seed):
    rng = np.random.default_rng(seed)
    return dict(d_actions=rng.standard_normal((K, T0, E0, 2 * M)), d_x0=rng.standard_normal((K, E0, N)),
                d_v0=rng.standard_normal((K, E0, N)))


@pytest.mark.parametrize("N", [N0, N1])
def test_kl_tangents_do_not_depend_on_the_launch_geometry(N):
    a = _actions(T0, E0, 9)
    feq = _feq(E0, 96, 96, True, 10, NARROW)
    u = _directions(3, N, 11)

    def run(every=0, envs=slice(None), **kw):
        env, X, V = _make(N=N, seed=6, **kw)
        if envs != slice(None):
            env.close()
            env, _, _ = _make(E=1, N=N, X=X[envs], V=V[envs], **kw)
        env.start_tape(T0, every, kl=_kl(feq[envs], NARROW))
        env.step_actions_traj(a[:, envs])
        out = env.tangent(kl=True, **{k: d[:, :, envs] if k == "d_actions" else d[:, envs] for k, d in u.items()})
        again = env.tangent(kl=True, **{k: d[:, :, envs] if k == "d_actions" else d[:, envs] for k, d in u.items()})
        assert all(np.array_equal(out[k], again[k]) for k in out)        # two calls on one tape: the same bits
        _healthy(env)
        sched = env._h.schedule()
        env.stop_tape()
        env.close()
        return out, sched

    ref, s0 = run()
    assert np.all(np.isfinite(ref["KL"])) and np.all(ref["KL"] != 0.0)
    if N == N0:
        assert s0 == "resident"
    for kw in (dict(blocks_per_env=1), dict(blocks_per_env=2), dict(every=1), dict(every=2)):
        got, sched = run(**kw)
        assert np.array_equal(got["KL"], ref["KL"]), kw
        if kw.get("blocks_per_env") == 2:
            assert sched == "streaming"
    alone, _ = run(envs=slice(1, 2))
    assert np.array_equal(alone["KL"][:, :, 0], ref["KL"][:, :, 1])


@pytest.mark.parametrize("K", [3, 8])
def test_k_directions_in_one_call_equal_k_calls(K):
    env, X, V = _make(N=N1 if K == 3 else N0, seed=7)
    N = env.N
    feq = _feq(E0, 32, 32, False, 12, WIDE)
    env.start_tape(T0, 2, kl=_kl(feq, WIDE))
    env.step_actions_traj(_actions(T0, E0, 13))
    u = _directions(K, N, 14)
    many = env.tangent(kl=True, **u)
    assert many["KL"].shape == (K, T0, E0)
    for k in range(K):
        one = env.tangent(kl=True, **{name: d[k] for name, d in u.items()})
        assert one["KL"].shape == (T0, E0)
        for key in one:
            assert np.array_equal(many[key][k], one[key]), (K, k, key)
    _healthy(env)
    env.stop_tape()
    env.close()


# ---- 6. nothing else moves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"blocks_per_env": 2}])
def test_the_kl_tangent_leaves_everything_else_alone(kw):
    rng = np.random.default_rng(15)
    a = _actions(T0, E0, 15)
    feq = _feq(E0, 32, 32, False, 16, WIDE)
    u = _directions(3, N0, 17)
    cot, kbar = rng.standard_normal((T0, 3, E0)), rng.standard_normal((T0, E0))
    bw = dict(d_KE=cot[:, 0], d_PE=cot[:, 1], d_PE_reward=cot[:, 2], d_KL=kbar)
    plain_env, _, _ = _make(**kw)
    plain_env.start_tape(T0, 2)
    plain_env.step_actions_traj(a)
    plain = plain_env.tangent(fields=True, **u)
    base = _healthy(plain_env)["launches"]
    plain_env.stop_tape()
    plain_env.close()
    env, _, _ = _make(**kw)
    env.start_tape(T0, 2, kl=_kl(feq, WIDE))
    env.step_actions_traj(a)
    trace = env.tape_kl()
    grad0 = env.backward(**bw)
    without = env.tangent(fields=True, **u)                               # a KL tape, kl = False: a plain tape's call
    assert _healthy(env)["launches"] == base
    assert set(without) == set(plain) and all(np.array_equal(without[k], plain[k]) for k in plain)
    before = [np.copy(p) for p in env.particles() + env.fields() + env.energies()]
    with_kl = env.tangent(fields=True, kl=True, **u)
    st = _healthy(env)
    assert st["launches"] == base + KL_LAUNCHES * T0 and st["steps"] == T0
    assert set(with_kl) == set(plain) | {"KL"}
    assert all(np.array_equal(with_kl[k], plain[k]) for k in plain)
    assert np.all(with_kl["KL"] != 0.0)
    for p, q in zip(env.particles() + env.fields() + env.energies(), before):
        assert np.array_equal(p, q)
    assert np.array_equal(env.tape_kl(), trace)
    grad1 = env.backward(**bw)                                            # the rows of pic_tape_kl_cot and the backward: as before
    assert all(np.array_equal(grad1[k], grad0[k]) for k in grad0)
    _healthy(env)
    env.stop_tape()
    env.close()


# ---- 7. the contract -----------------------------------------------------------------------------------------------------------
def test_contract():
    from ocplasma_amd._abi import PIC_HOST, PicError
    a = _actions(T0, E0, 18)
    feq = _feq(E0, 24, 40, False, 19, WIDE)
    u = _directions(1, N0, 20)
    one = {k: d[0] for k, d in u.items()}
    env, X, V = _make()
    h = env._h
    buf = np.full((1, T0, E0), 7.0)

    def raw(K=1, kl=buf, **ins):                                          # pic_tape_tangent_kl itself, host memory
        h._tape_tangent(PIC_HOST, K, *(ins[k].ctypes.data if k in ins else 0 for k in ("d_ext", "d_actions", "d_x0", "d_v0")),
                        0, 0, 0, 0, kl=kl.ctypes.data)

    # no KL on the tape: refused with the reason, by the library and by the Python layer
    env.start_tape(T0, 2)
    env.step_actions_traj(a)
    with pytest.raises(PicError, match="needs a KL on the tape"):
        raw(d_x0=u["d_x0"])
    with pytest.raises(PicError, match="needs a KL on the tape"):
        env.tangent(kl=True, **one)
    assert "KL" not in env.tangent(**one)
    env.stop_tape()
    # T = 0: nothing is written
    env.reset(X, V)
    env.start_tape(T0, 2, kl=_kl(feq, WIDE))
    raw(d_x0=u["d_x0"])
    assert np.all(buf == 7.0)
    assert env.tangent(kl=True, d_x0=one["d_x0"])["KL"].shape == (0, E0)
    env.step_actions_traj(a)
    # K = 9, and both d_ext and d_actions: refused as before
    with pytest.raises(PicError, match="-1"):
        raw(K=9, kl=np.zeros((9, T0, E0)))
    with pytest.raises(PicError, match="-1"):
        raw(d_ext=np.zeros((1, T0, E0, NG0)), d_actions=u["d_actions"])
    with pytest.raises(PicError, match="-1"):
        h.phase_kl_smooth_jvp(24, 40, *WIDE, feq.ctypes.data, 0, PIC_HOST, 9, 0, 0, PIC_HOST, np.zeros((9, E0)).ctypes.data)
    with pytest.raises(PicError, match="-1"):
        h.phase_kl_smooth_jvp(24, 40, *WIDE, 0, 0, PIC_HOST, 1, 0, 0, PIC_HOST, np.zeros((1, E0)).ctypes.data)      # no feq
    # the memory: the tangent block of one direction, then the KL's part by the header's formula
    plain_bytes = env.tape_stats()["bytes"]
    env.tangent(**one)
    tan_bytes = env.tape_stats()["bytes"]
    assert tan_bytes > plain_bytes
    host = env.tangent(kl=True, **one)
    want = _kl_part_bytes(E0, N0)
    assert env.tape_stats()["bytes"] == tan_bytes + want
    env.tangent(kl=True, **one)
    assert env.tape_stats()["bytes"] == tan_bytes + want                  # allocated once
    # host and device memory: the same bits
    dev = env.tangent(kl=True, **{k: torch.as_tensor(d, device="cuda") for k, d in one.items()})
    assert dev["KL"].is_cuda and all(np.array_equal(dev[k].cpu().numpy(), host[k]) for k in host)
    grad = env.backward(d_KL=np.ones((T0, E0)))
    env.stop_tape()
    # one byte short of the KL's part: PIC_ENOMEM, and the tape stays usable; exactly enough passes
    for budget, fits in ((tan_bytes + want - 1, False), (tan_bytes + want, True)):
        env.reset(X, V)
        env.start_tape(T0, 2, budget_bytes=budget, kl=_kl(feq, WIDE))
        env.step_actions_traj(a)
        if fits:
            got = env.tangent(kl=True, **one)
        else:
            with pytest.raises(PicError, match="-4"):
                env.tangent(kl=True, **one)
            assert env.tape_stats()["bytes"] == tan_bytes
            got = env.tangent(**one)
        assert all(np.array_equal(got[k], host[k]) for k in got)
        again = env.backward(d_KL=np.ones((T0, E0)))
        assert all(np.array_equal(again[k], grad[k]) for k in grad)
        _healthy(env)
        env.stop_tape()
    env.close()
    # a gain-law tape is still refused
    import hp_feedback as hf
    e3, _, _ = _make(E=1, N=2000, seed=8)
    e3.start_tape(3, kl=_kl(_feq(1, 24, 40, False, 21, WIDE), WIDE))
    e3.step_feedback_gain(hf.g0(M), 3)
    with pytest.raises(PicError, match="gain law"):
        e3.tangent(kl=True, d_x0=np.ones((1, 2000)))
    e3.stop_tape()
    e3.close()


# ---- 8. torch ------------------------------------------------------------------------------------------------------------------
def test_torch_forward_ad_carries_the_kl_tangent():
    import torch.autograd.forward_ad as fwAD
    from ocplasma_amd.env import grad
    feq = _feq(E0, 32, 32, False, 22, WIDE)
    env, X, V = _make(seed=9)
    a = torch.tensor(_actions(T0, E0, 23), dtype=torch.float64, device="cuda")
    du = torch.tensor(np.random.default_rng(24).standard_normal((T0, E0, 2 * M)), dtype=torch.float64, device="cuda")
    with fwAD.dual_level():
        outs = grad.rollout(env, fwAD.make_dual(a, du), kl=_kl(feq, WIDE))
        assert len(outs) == 4
        tans = [fwAD.unpack_dual(o).tangent for o in outs]
    ref = env.tangent(d_actions=du, kl=True)
    plain = env.tangent(d_actions=du)
    for t, k in zip(tans, ("KE", "PE", "PE_reward", "KL")):
        assert torch.equal(t, ref[k]), k
    assert bool((tans[3] != 0).all())                                     # (zero before pic_tape_tangent_kl existed)
    for k in ("KE", "PE", "PE_reward"):
        assert torch.equal(ref[k], plain[k]), k                           # the energy tangents: unchanged
    _healthy(env)
    env.stop_tape()
    # raw fields, host tensors
    env.reset(X, V)
    e = torch.tensor(_ext_of(a.cpu().numpy(), NG0))
    de = torch.tensor(0.1 * np.random.default_rng(25).standard_normal((T0, E0, NG0)))
    with fwAD.dual_level():
        tans = [fwAD.unpack_dual(o).tangent for o in grad.rollout_ext(env, fwAD.make_dual(e, de), kl=_kl(feq, WIDE))]
    ref = env.tangent(d_ext=de.numpy(), kl=True)
    for t, k in zip(tans, ("KE", "PE", "PE_reward", "KL")):
        assert np.array_equal(t.numpy(), ref[k]), k
    assert np.all(ref["KL"] != 0.0)
    env.stop_tape()
    env.close()
