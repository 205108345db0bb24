"""The other integrators on the device (include/picstep.h: pic_set_integrator): symplectic Euler, Stormer-Verlet
and forward Euler against the reference's own runs (G18) and against tests/hp_integrators.py step by step, bit identity across
call shapes, geometry, the recorder and scheme switches, and the sweep counts the feature exists for.

Golden bounds (G18, float64) are 100 x the worst error measured on an MI355X over all cases, schemes and schedules (the
project's convention; every value is recorded with record_measure): positions / L and velocities relative to max|v|, over the
particles G18 keeps (every mark_stride-th), after step 1: 7.7e-16, step 10: 6.1e-15, the last step (200 / 100 / 50 / 20):
6.1e-14; the total-energy trace, which every particle enters: 5.1e-15.  The two sides round differently in the deposit
(fixed-point sums) and the solve (scans against Sherman-Morrison)."""
import numpy as np
import pytest

import hp_checks as hc
import hp_integrators as hpi
from conftest import circ_err, load_golden, record_measure, rel_err

pytestmark = pytest.mark.gpu

SCHEMES = ("symplectic_euler", "verlet", "forward_euler")
TAGS = {"symplectic_euler": "se", "verlet": "vv", "forward_euler": "fe"}
FORMATS = [("float64", None), ("float32", None), ("float32", "fixed32")]
TOL_1, TOL_10, TOL_LAST, TOL_H = 7.7e-14, 6.2e-13, 6.1e-12, 5.1e-13


@pytest.fixture(scope="module")
def oc():
    import ocplasma_amd
    return ocplasma_amd


@pytest.fixture(scope="module")
def g18():
    return load_golden("g18_integrators")


def _case(g, pre):
    N, Ng, dt, K = int(g[f"{pre}_N"]), int(g[f"{pre}_Ng"]), float(g[f"{pre}_dt"]), int(g[f"{pre}_steps"])
    return N, Ng, dt, K, ("TSC" if bool(g[f"{pre}_tsc"]) else "CIC")


def _ext_traj(oc, g, pre, L, Ng, K):
    """[K, Ng] external field of every step (None: none)"""
    if f"{pre}_E_ext" in g.files:
        return np.repeat(g[f"{pre}_E_ext"].reshape(1, Ng), K, axis=0)
    if f"{pre}_actions" in g.files:
        act = oc.E_field(L, Ng, 3)
        out = []
        for a in g[f"{pre}_actions"]:
            act.update_E(a[:3], a[3:])
            out.append(np.asarray(act.compute_E()).ravel())
        return np.array(out)
    return None


def _compare(g, pre, tag, k, x, v, L, what):
    """x, v after step k against G18's, which keeps every mark_stride-th particle of them"""
    xr, vr = g[f"{pre}_{tag}_x_{k}"], g[f"{pre}_{tag}_v_{k}"]
    ms = int(g["mark_stride"])
    tol = TOL_1 if k == 1 else (TOL_10 if k == 10 else TOL_LAST)
    ex, ev = circ_err(np.asarray(x)[::ms], xr, L) / L, rel_err(np.asarray(v)[::ms], vr)
    record_measure(f"integrators.golden.{what}.{pre}.{tag}.step{k}", max(ex, ev))
    assert ex < tol and ev < tol, (what, pre, tag, k, ex, ev)


# -- 1. golden parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", ["ts", "bot", "ext", "act"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_golden_through_pic(oc, g18, pre, scheme):
    """PIC with the reference's own function object (its __name__ selects the scheme), stepped one update_state at a time."""
    L = float(g18["L"])
    N, Ng, dt, K, shape = _case(g18, pre)
    tag = TAGS[scheme]
    fn = lambda eta, grad, dt: eta   # noqa: E731
    fn.__name__ = scheme
    sim = oc.PIC(N=N, N_mesh=Ng, n0=1.0, L=L, dt=dt, A=0.1, n_mode=2, interpol=shape,
                 init_dist=oc.TwoStream(3.0, 1.0, N, L), integrator=fn)
    sim.x = g18[f"{pre}_x_init"].reshape(-1, 1)
    sim.v = g18[f"{pre}_v_init"].reshape(-1, 1)
    ext = _ext_traj(oc, g18, pre, L, Ng, K)
    H = []
    for k in range(1, K + 1):
        sim.update_state(None if ext is None else ext[k - 1].reshape(-1, 1))
        H.append(sim.get_energy())
        if k in (1, 10, K):
            _compare(g18, pre, tag, k, sim.x.ravel(), sim.v.ravel(), L, "pic")
            if k == 1:
                assert rel_err(sim.E_mesh.ravel(), g18[f"{pre}_{tag}_E_mesh_1"]) < 1e3 * TOL_1
    eh = rel_err(H, g18[f"{pre}_{tag}_H"][1:])
    record_measure(f"integrators.golden.pic.{pre}.{tag}.H", eh)
    assert eh < TOL_H


@pytest.mark.parametrize("pre,bpe", [(p, b) for p in ("ts", "bot", "ext", "act") for b in (-1, 2) if not (p == "bot" and b == -1)])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_golden_through_batched(oc, g18, pre, scheme, bpe):
    """BatchedPIC, two identical environments, resident (bpe = -1) and streaming (bpe = 2): calls of 1, 9 and K - 10 steps.
    (The bump-on-tail case, N = 1e4, is beyond the resident schedule's 8192 particles: streaming only.)"""
    L = float(g18["L"])
    N, Ng, dt, K, shape = _case(g18, pre)
    tag = TAGS[scheme]
    env = oc.BatchedPIC(2, N, Ng, L=L, dt=dt, interpol=shape, blocks_per_env=bpe, integrator=scheme)
    assert env._h.schedule() == ("resident" if bpe == -1 else "streaming")
    env.reset(np.tile(g18[f"{pre}_x_init"], (2, 1)), np.tile(g18[f"{pre}_v_init"], (2, 1)))
    ext = _ext_traj(oc, g18, pre, L, Ng, K)
    done = 0
    KE, PE = [], []
    for k in (1, 10, K):
        n = k - done
        if ext is None:
            ke, pe, _ = env.step_history(None, n)
        elif f"{pre}_E_ext" in g18.files:
            ke, pe, _ = env.step_history(np.tile(ext[0], (2, 1)), n)
        else:
            ke, pe, _ = env.step_ext_traj(np.repeat(ext[done:k, None, :], 2, axis=1), history=True)
        KE.append(ke[:, 0]); PE.append(pe[:, 0])
        done = k
        x, v = env.particles()
        assert np.array_equal(x[0], x[1]) and np.array_equal(v[0], v[1])
        _compare(g18, pre, tag, k, x[0], v[0], L, f"batched{bpe}")
    eh = rel_err(np.concatenate(KE) + np.concatenate(PE), g18[f"{pre}_{tag}_H"][1:])
    record_measure(f"integrators.golden.batched{bpe}.{pre}.{tag}.H", eh)
    assert eh < TOL_H


# -- 2. step-local matrix against hp_integrators ------------------------------------------------------------------------------
def scheme_push_bound(c, scheme, pre, info, E_ext_err):
    """Per-particle bounds (dx, dv) on one device step from `pre` against hp_integrators.scheme_step from the same state.  The
    terms are hp_checks.push_bound's, event by event (force evaluation k uses info["E"][k] at the positions of that moment):
      field at the particle:  dEp <= wsum dE_mesh + max|E| (n_w (w_err + Lip dq / dx) + (2 n_w + 2) u_W)   [+3 max|E| TSC edge]
        dE_mesh <= 2 dx sum_j dn_j + (5m + 26) u64 (sum|b| dx) + 2 u64 max|E| + E_ext_err,
        dn_j <= count_j (w_err + quantum + Lip dq / dx) scale + 6 u64 |n_j|
      kick  p + (d (-E)) dt:   dp += |d| dt dEp + 4 u_V (|p| + |d Ep dt|)       (d = 1, or 0.5 for Verlet's half-kicks)
      drift q + (c p) dt:      dq += |c| dt dp + 4 u_X (|q| + |c p dt|); fixed point 4 u32 |c p dt| + L 2^-33
      forward Euler drifts with the velocity before the kick (its dp is 0: the state is exact), then kicks.
    The wrap adds u_X L (float formats)."""
    u = hc._u(c)
    dt = float(c.dt)
    dx = c.L / c.Ng
    scale = c.n0 * c.L / c.N / dx
    nw = 2 if c.shape == "CIC" else 3
    lip = 1.0 if c.shape == "CIC" else 2.0
    wsum = 1.0 if c.shape == "CIC" else 1.6
    N = pre["v"].size
    dq = np.zeros(N)
    dp = np.zeros(N)
    q_at = [hpi.fixed_to_length(pre["x"], c.L) if c.fixed else hpi.as_ld(pre["x"])] + list(info["q"])
    u_x = hc.U32 if c.fixed else u

    def field_err(k):
        Em, Ep, n_hp, count = info["E"][k]
        dqmax = float(np.max(dq))
        per = hc._weight_err(c) + hc._quantum(c) + lip * dqmax / dx
        cnt = count.astype(float)
        dn = cnt * per * scale + 6 * hc.U64 * np.abs(n_hp.astype(float))
        amb = np.zeros(N, dtype=bool)
        if c.shape == "TSC":
            qc = hpi.wrap(q_at[k], c.L) / hpi.LD(dx)
            dist = np.abs(qc - np.round(qc)).astype(float)
            amb = dist <= (dq / dx + (2 * c.Ng + 4) * u + 1e-15)
            if amb.any():
                jf = np.floor(qc[amb]).astype(np.int64)
                for o in (-2, -1, 0, 1, 2):
                    np.add.at(dn, np.mod(jf + o, c.Ng), 3.0 * scale)
        Emax = float(np.max(np.abs(Em)))
        m = (c.Ng + 63) // 64
        sb = float(np.sum(np.abs(n_hp.astype(float) - c.n0))) * dx + float(np.sum(dn)) * dx
        dE_mesh = 2 * dx * float(np.sum(dn)) + (5 * m + 26) * hc.U64 * sb + 2 * hc.U64 * Emax + E_ext_err
        dEp = wsum * dE_mesh + Emax * (nw * (hc._weight_err(c) + lip * dq / dx) + (2 * nw + 2) * u)
        return dEp + np.where(amb, 3.0 * Emax, 0.0), np.abs(Ep.astype(float))

    def kick(d, k, p_after):
        nonlocal dp
        dEp, Ep = field_err(k)
        dp = dp + d * dt * dEp + 4 * u * (np.abs(p_after.astype(float)) + d * Ep * dt)

    def drift(q_after, p_used):
        nonlocal dq
        disp = np.abs(p_used.astype(float)) * dt
        if c.fixed:
            dq = dq + dt * dp + 4 * hc.U32 * disp + c.L * 2.0 ** -33
        else:
            dq = dq + dt * dp + 4 * u_x * (np.abs(q_after.astype(float)) + disp)

    if scheme == "forward_euler":
        drift(info["q"][0], hpi.as_ld(pre["v"]))
        kick(1.0, 0, info["p"][0])
    elif scheme == "symplectic_euler":
        kick(1.0, 0, info["p"][0])
        drift(info["q"][0], info["p"][0])
    else:
        kick(0.5, 0, info["p"][0])
        drift(info["q"][0], info["p"][0])
        kick(0.5, 1, info["p"][1])
    if not c.fixed:
        dq = dq + u * c.L
    return dq, dp


def _plant(x, L, rng):
    """edge, far and fast positions / velocities in the first particles (hp_checks' planted cases, in brief)"""
    x[0], x[1], x[2] = 0.0, np.nextafter(L, 0.0), L / 2
    return x


MATRIX = [(s, d, p, sh, bpe) for s in SCHEMES for (d, p) in FORMATS for sh in ("CIC", "TSC") for bpe in (-1, 3)]


@pytest.mark.parametrize("scheme,dtype,pos,shape,bpe", MATRIX)
def test_step_local_against_hp(oc, scheme, dtype, pos, shape, bpe):
    """One step from the device's own state, every environment, against hp_integrators with the bounds of scheme_push_bound;
    the state after it against hp_reference (hp_checks.check_stages).  Ragged N, the singular mesh L = 50, Ng = 100, an
    external field on one environment, planted edge / fast particles."""
    N, Ng, L, E_ = 3001, 100, 50.0, 2
    env = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, dtype=dtype, position_dtype=pos, interpol=shape, blocks_per_env=bpe,
                        integrator=scheme)
    rng = np.random.default_rng(5)
    x = rng.uniform(0, L, (E_, N))
    v = rng.normal(0, 1.0, (E_, N)) + np.where(rng.uniform(size=(E_, N)) < 0.5, 3.0, -3.0)
    for e in range(E_):
        _plant(x[e], L, rng)
    v[:, 3] = 40.0                                        # fast: 4 cells in one step
    env.reset(x, v)
    env.step(None, 1)                                     # a step from the device's own state first
    ext = np.zeros((E_, Ng))
    ext[1] = 0.3 * np.sin(2 * np.pi * np.arange(Ng) / Ng)
    c = hc.Case(dtype, pos or "float", shape, N, Ng, L, E_, None, n0=1.0, dt=env.dt)
    views = env.torch_views()
    pre = [hc._read(env, c, e, views) for e in range(E_)]
    env.step(ext, 1)
    for e in range(E_):
        post = hc._read(env, c, e, views)
        tag = f"{scheme} {c} env {e}"
        hc.check_stages(c, post, tag)
        x1, v1, info = hpi.scheme_step(scheme, pre[e]["x"], pre[e]["v"], ext[e], c.dt, Ng, L, 1.0, N, shape, hc._cell_dtype(c))
        bq, bp = scheme_push_bound(c, scheme, pre[e], info, 0.0)
        xd = hpi.fixed_to_length(post["x"], L) if c.fixed else hpi.as_ld(post["x"])
        d = np.abs(xd - x1)
        d = np.minimum(d, hpi.LD(L) - d).astype(float)
        dv = np.abs(hpi.as_ld(post["v"]) - v1).astype(float)
        record_measure(f"integrators.local.{scheme}.{dtype}.{pos}.{shape}.x", float(np.max(d / bq)))
        record_measure(f"integrators.local.{scheme}.{dtype}.{pos}.{shape}.v", float(np.max(dv / bp)))
        assert np.all(d <= bq), (tag, "x", float(np.max(d / bq)))
        assert np.all(dv <= bp), (tag, "v", float(np.max(dv / bp)))


# -- 3. bit identity across call shapes -----------------------------------------------------------------------------------------
def _state(env):
    x, v = env.particles()
    return [x, v] + list(env.fields()) + list(env.energies())


def _same(a, b, what, skip_ke=False):
    for i, (p, q) in enumerate(zip(a, b)):
        if skip_ke and i == 5:
            continue
        assert np.array_equal(p, q), (what, i)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype,pos", FORMATS)
@pytest.mark.parametrize("N,bpe", [(20000, 0), (3000, 0)])
def test_call_shapes_bit_identical(oc, scheme, dtype, pos, N, bpe):
    """K steps in one call == K one-step calls == S staged calls per step, for pic_step, history, actions_traj (a new action
    every step), feedback and observe.  (N = 20000 streams, N = 3000 is resident.)"""
    E_, Ng, L, K = 2, 64, 50.0, 5
    act = oc.E_field(L, Ng, 3)
    rng = np.random.default_rng(3)
    acts = rng.uniform(-1, 1, (K, E_, 6))
    envs = []
    for _ in range(3):
        env = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, dtype=dtype, position_dtype=pos, blocks_per_env=bpe, integrator=scheme)
        env.set_actuator(act)
        env.reset_sampled(seed=11)
        envs.append(env)
    a, b, c = envs
    S = a._h.integrator()[1]
    a.step(None, K)
    for _ in range(K):
        b.step(None, 1)
        for s in range(1, S + 1):
            c._h.step_stage(s, None)
    _same(_state(a), _state(b), "step K vs 1")
    _same(_state(a), _state(c), "step vs staged", skip_ke=N <= 8192)   # (staged steps of a resident handle run as sweeps)
    ha = a.step_history(None, K)
    hb = [b.step_history(None, 1) for _ in range(K)]
    for i in range(3):
        assert np.array_equal(ha[i], np.concatenate([h[i] for h in hb])), ("history", i)
    _same(_state(a), _state(b), "history")
    a.step_actions_traj(acts)
    for k in range(K):
        b.step_actions_traj(acts[k:k + 1])
    _same(_state(a), _state(b), "actions_traj")
    fa = a.step_feedback(K, actions=True, history=True)
    fb = [b.step_feedback(1, actions=True, history=True) for _ in range(K)]
    assert np.array_equal(fa["actions"], np.concatenate([f["actions"] for f in fb]))
    _same(_state(a), _state(b), "feedback")
    sa = a.step_observe(actions=acts[0], nsteps=K)
    for _ in range(K):
        sb = b.step_observe(actions=acts[0], nsteps=1)
    assert np.array_equal(sa[0], sb[0])
    _same(_state(a), _state(b), "observe")


# -- 4. geometry: resident == streaming, any blocks_per_env ----------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype,pos", FORMATS)
@pytest.mark.parametrize("shape", ["CIC", "TSC"])
def test_geometry_bit_identical(oc, scheme, dtype, pos, shape):
    E_, N, Ng, L = 1, 5000, 250, 50.0
    out = []
    for bpe in (-1, 1, 3, 0):
        env = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.05, dtype=dtype, position_dtype=pos, interpol=shape, blocks_per_env=bpe,
                            integrator=scheme)
        env.reset_sampled("two-stream", seed=4)
        env.step(None, 7)
        env.step_history(None, 3)
        out.append(_state(env))
    for o in out[1:]:
        _same(out[0], o, "geometry", skip_ke=True)     # KE: a float64 sum whose order follows the launch grid


# -- 5. recorder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("N", [20000, 3000])
def test_recorder_does_not_perturb(oc, scheme, N):
    E_, Ng, L = 2, 64, 50.0
    envs = []
    for rec in (False, True):
        env = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, integrator=scheme)
        env.reset_sampled(seed=21)
        if rec:
            env.start_recording(stride=3, x_bins=16, v_bins=16, capacity=16)
        envs.append(env)
    for env in envs:
        env.step(None, 7)
        env.step_history(None, 4)
    _same(_state(envs[0]), _state(envs[1]), "recorder")
    rec = envs[1].recorded()
    assert list(rec.steps) == [3, 6, 9]


# -- 6. launch counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("K", [1, 5, 20])
def test_sweeps_per_call(oc, scheme, K):
    """A K-step Verlet call launches at most K + 1 particle sweeps; symplectic and forward Euler K, plus a first-deposit sweep
    where one is due (after set_particles, which leaves no deposit)."""
    env = oc.BatchedPIC(2, 20000, 64, L=50.0, dt=0.1, integrator=scheme)
    env.reset_sampled(seed=2)
    env.step(None, 1)
    env.profile(True)
    env.step(None, K)
    env.sync()
    prof = env.profile_read()
    sweeps = sum(n for k, (_, n) in prof.items() if k.startswith("sweep"))
    assert sweeps == (K + 1 if scheme == "verlet" and K > 1 else (2 * K if scheme == "verlet" else K)), prof
    x, v = env.particles()
    env._h.set_particles(x, v)
    env.profile(False)
    env.profile(True)
    env.step(None, K)
    env.sync()
    prof = env.profile_read()
    assert prof["sweep_aux"][1] == 1
    assert prof["sweep_integrator"][1] == (K + 1 if scheme == "verlet" and K > 1 else (2 * K if scheme == "verlet" else K))


def test_launches_match_schedule(oc):
    """One launch per descriptor of the step schedule: the launches per profile kind of reset, step(1), step(3), step_history(2),
    read-only C with step(3), then Verlet with step(3) are the counts tests/schedule_driver.cpp prints for the script
    "0 0 0 i r s1 s3 s2 o1 s3 k2 s3" (tests/test_schedule_cpu.py::test_gpu_script_launch_counts holds the driver to them)."""
    E, N, Ng, L = 2, 3000, 64, 50.0
    env = oc.BatchedPIC(E, N, Ng, L=L, dt=0.1, blocks_per_env=2)
    assert env._h.schedule() == "streaming"
    rng = np.random.default_rng(11)
    env.profile(True)
    env.reset(rng.uniform(0.0, L, (E, N)), rng.normal(0.0, 1.0, (E, N)))
    env.step(None, 1)
    env.step(None, 3)
    env.step_history(None, 2)
    env._h.set_readonly_c("on")
    env.step(None, 3)
    env._h.set_integrator("verlet")
    env.step(None, 3)
    env.sync()
    prof = {k: n for k, (_, n) in env.profile_read().items()}
    env.close()
    # (profile_read leaves out the kinds that never ran: no sweep A, no resident launch)
    assert prof == {"sweep_B": 9, "sweep_C": 9, "sweep_D": 9, "field_solve": 8, "sweep_aux": 2, "sweep_integrator": 4}, prof


# -- 7. switching schemes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("bpe", [-1, 2])
def test_switch_equals_fresh_handle(oc, scheme, bpe):
    E_, N, Ng, L = 2, 4000, 128, 50.0
    a = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, blocks_per_env=bpe)
    a.reset_sampled(seed=8)
    a.step(None, 3)
    x, v = a.particles()
    a._h.set_integrator(scheme)
    assert a._h.integrator()[0] == scheme
    a.step(None, 4)
    b = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, blocks_per_env=bpe, integrator=scheme)
    b.reset(x, v)
    b.step(None, 4)
    _same(_state(a), _state(b), "switch")
    a._h.set_integrator("symplectic_4th_order")        # and back: a fresh Yoshida-4 handle from the same state
    x, v = a.particles()
    a.step(None, 2)
    c = oc.BatchedPIC(E_, N, Ng, L=L, dt=0.1, blocks_per_env=bpe)
    c.reset(x, v)
    c.step(None, 2)
    _same(_state(a), _state(c), "switch back")


def test_stage_rules(oc):
    env = oc.BatchedPIC(1, 3000, 64, L=50.0, dt=0.1, integrator="verlet")
    env.reset_sampled(seed=1)
    env._h.step_stage(1, None)
    with pytest.raises(oc._abi.PicError, match="staged step"):
        env._h.set_integrator("symplectic_euler")
    with pytest.raises(oc._abi.PicError):
        env._h.step_stage(3, None)
    env._h.step_stage(2, None)
    with pytest.raises(oc._abi.PicError):
        env._h.set_integrator(7)
    env._h.set_integrator("symplectic_euler")
    with pytest.raises(oc._abi.PicError):
        env._h.step_stage(2, None)
    env._h.step_stage(1, None)


def test_pic_input_func_and_update_params(oc):
    """update_state_w_input_func calls the input function once per force evaluation; update_params(integrator=...) re-creates
    the handle and keeps the particles."""
    calls = []
    sim = oc.PIC(N=3000, N_mesh=64, L=50.0, dt=0.1, init_dist=oc.TwoStream(3.0, 1.0, 3000, 50.0), integrator="verlet")
    sim.update_state_w_input_func(lambda eta: calls.append(eta.shape) or None)
    assert len(calls) == 2
    x = sim.x.copy()
    sim.update_params(integrator="forward_euler")
    assert np.array_equal(sim.x, x)
    calls.clear()
    sim.update_state_w_input_func(lambda eta: calls.append(eta.shape) or None)
    assert len(calls) == 1
    with pytest.raises(ValueError):
        sim.update_params(integrator="implicit_midpoint")


# -- 8. default unchanged --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [20000, 3000])
def test_explicit_yoshida_equals_default(oc, N):
    a = oc.BatchedPIC(2, N, 64, L=50.0, dt=0.1)
    b = oc.BatchedPIC(2, N, 64, L=50.0, dt=0.1, integrator="symplectic_4th_order")
    b._h.set_integrator(oc._abi.PIC_YOSHIDA4)
    assert a._h.integrator() == ("symplectic_4th_order", 3)
    for env in (a, b):
        env.reset_sampled(seed=6)
        env.step(None, 6)
        env.step_history(None, 2)
    _same(_state(a), _state(b), "default")
