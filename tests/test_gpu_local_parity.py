"""Step-local differential matrix: every stage of a step, for every particle format, shape, accumulator, schedule and a spread of
(N, Ng, L), checked against tests/hp_reference.py (longdouble) starting from the device's own state before that step.

Because each step starts from the device's state, the bounds do not grow with the step count or with the chaos of the system;
they are derived from the arithmetic (see `density_bound`, `solve_bounds`, `push_bound`, `energy_bounds`), not fitted, and
every measured / bound ratio is recorded with record_measure.  A twin handle runs the same steps as ONE multi-step call
(`step_history`) so that the hand-over between the inner steps of a call is covered too: its energies after every inner step
and its final state are checked against the reference evaluated on the single-stepping handle's states.
"""
import zlib

import numpy as np
import pytest

import hp_reference as hp
from conftest import record_measure
from hp_checks import (U64, Case, _acc_kind, _fg, _planted_positions, _ratio, _read, check_energies_of, check_push,
                       check_stages)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _matrix():
    """Explicit rows (each row of the issue's matrix is hit at least once); the pairings of L, E_ext and actions are spread
    with a fixed seed."""
    rng = np.random.default_rng(20261015)
    F64, F32, U = ("float64", "float"), ("float32", "float"), ("float32", "fixed32")
    rows = [
        # (format, shape, N, Ng, envs, accum, bpe, planted)
        (F64, "CIC", 1, 4, 2, None, -1, None),
        (F32, "TSC", 3, 5, 2, None, -1, None),
        (U, "CIC", 63, 63, 1, None, -1, "edges"),
        (F64, "TSC", 64, 64, 1, None, 0, "edges"),
        (F32, "CIC", 65, 65, 2, "packed", 3, "edges"),
        (U, "TSC", 1023, 127, 1, None, 0, None),
        (F64, "CIC", 1025, 128, 1, "float64", 2, None),
        (F32, "TSC", 2047, 129, 1, "fix64", 0, None),
        (F32, "CIC", 2049, 511, 2, None, -1, "far_reset"),
        (F64, "CIC", 2048, 512, 1, "fix64", -1, "far_set"),
        (U, "CIC", 4095, 513, 1, "fix64", 2, "far_reset"),
        (F64, "TSC", 4096, 1023, 1, None, 0, "fast"),
        (F32, "CIC", 4097, 1024, 1, None, 2, "far_set"),
        (U, "TSC", 5120, 1025, 1, None, 0, "edges"),
        (F64, "CIC", 8192, 100, 1, "float64", 3, "edges"),
        (F32, "TSC", 8193, 300, 1, None, 0, "fast"),
        (F64, "TSC", 3000, 1159, 1, None, -1, None),
        (F32, "CIC", 3001, 1249, 1, None, -1, None),
        (F64, "CIC", 3000, 2722, 1, None, 2, "edges"),
        (F32, "TSC", 3003, 3267, 1, None, 2, None),
        (U, "CIC", 3000, 3267, 1, None, 3, None),
        (F64, "CIC", 20000, 2039, 3, None, 0, None),
        (F64, "TSC", 70000, 64, 1, None, 64, None),           # one environment, 35 workgroups: S = 4 accumulator sub-rows
        (F32, "CIC", 40001, 256, 2, None, 32, None),          # two environments, 20 workgroups each: S = 2
        (U, "CIC", 1 << 20, 64, 1, "fix64", 0, None),
    ]
    cases = []
    for (dtype, pos), shape, N, Ng, envs, accum, bpe, planted in rows:
        if bpe == 2 and N > 4096:
            bpe = int(rng.integers(2, 6))
        L = float(rng.choice([1.0, 10.0, 50.0, 77.7]))
        if Ng in (100, 300):
            L = 50.0                       # singular in the reference's Sherman-Morrison solve
        ext = bool(rng.integers(0, 2))
        actions = (not ext) and bool(rng.integers(0, 2))
        dt = float(rng.choice([0.02, 0.05, 0.1]))
        cases.append(Case(dtype, pos, shape, N, Ng, L, envs, accum, bpe, ext, actions, planted, dt=dt,
                          check_envs=2 if envs > 1 and N <= 70000 else 1))
    # an HBM-resident state (>= 256 MB of particles): multi-step calls hand the post-step deposit over to the next step's sweep
    cases.append(Case("float64", "float", "CIC", 1_000_000, 256, 50.0, envs=17, dt=0.01, sampled=True, check_envs=1))
    return cases


CASES = _matrix()


# ---------------------------------------------------------------------------------------------------------------------
# device state
# ---------------------------------------------------------------------------------------------------------------------
def _make(oc, c):
    return oc.BatchedPIC(c.envs, c.N, c.Ng, n0=c.n0, L=c.L, dt=c.dt, interpol=c.shape, dtype=c.dtype, accum_dtype=c.accum,
                         blocks_per_env=c.bpe, position_dtype=c.pos)


def _initial_state(c, rng):
    x0 = rng.uniform(0, c.L, (c.envs, c.N))
    v0 = rng.normal(0, 1, (c.envs, c.N))
    if c.planted in ("edges", "far_reset", "far_set", "fast"):
        if c.planted == "edges":
            pts = _planted_positions(c, rng)
        elif c.planted in ("far_reset", "far_set"):
            far = 1e3 * c.L + rng.uniform(0, c.L, 16)
            pts = np.concatenate([far, -far])
        else:
            pts = rng.uniform(0, c.L, 8)
        m = min(pts.size, c.N)
        x0[:, :m] = pts[:m]
        if c.planted == "fast":
            # carried more than one box length in ONE sub-stage (|c1 v dt| > L): wrap_periodic_far on the hot path
            cs, _ = hp.yoshida4_coefficients()
            v0[:, :m] = np.where(np.arange(m) % 2, 1, -1) * 2.5 * c.L / (float(cs[0]) * c.dt) * (1 + rng.uniform(0, 1, m))
    return x0.astype(c.dtype), v0.astype(c.dtype)


def _check_loaded(c, env, x0, views):
    """After a refresh the float formats hold np.mod(np.mod(x0, L), L) bit for bit, fixed32 the rounding of pos_from_length."""
    for e in range(c.check_envs):
        env.sync()
        if c.fixed:
            got = views["x_fixed"][e].cpu().numpy().view(np.uint32)
            xs = x0[e].astype(np.float64)
            r = xs - np.floor(xs / c.L) * c.L
            r = np.where((r >= 0) & (r < c.L), r, 0.0)
            want = (np.rint(r / c.L * 4294967296.0).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            assert np.array_equal(got, want), (c, e)
        else:
            W = np.dtype(c.dtype).type
            got = views["x"][e].cpu().numpy()
            want = np.mod(np.mod(x0[e], W(c.L)), W(c.L))
            # bytes, not values: -0.0 loaded must come out as np.mod's +0.0
            assert np.array_equal(got.view(np.uint8), want.astype(c.dtype).view(np.uint8)), (c, e)


# ---------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------
def _controls(oc, c, rng, envs):
    """(per-step E_ext given to the device, the same for the reference per environment, error bound of E_ext's rounding)."""
    if c.ext:
        E = rng.uniform(-0.5, 0.5, (envs, c.Ng))
        return ("ext", E), E, 0.0
    if c.actions:
        M = 3
        act = oc.E_field(c.L, c.Ng, M)
        a = rng.uniform(-1.25, 1.25, (envs, 2 * M))
        E = act.compute_E_batched(a)
        # device: sum_m bc[j, m] a[m] then the sin half, added (2M additions) -- the host mirror's order may differ
        mag = np.abs(act.basis_cos) @ np.abs(a[:, :M]).T + np.abs(act.basis_sin) @ np.abs(a[:, M:]).T
        return ("act", act, a), E, (2 * M + 2) * U64 * float(np.max(mag))
    return None, None, 0.0


def _step(env, ctl, nsteps=1, history=False):
    if ctl is None:
        return env.step_history(None, nsteps) if history else env.step(None, nsteps)
    if ctl[0] == "ext":
        return env.step_history(ctl[1], nsteps) if history else env.step(ctl[1], nsteps)
    env.step_actions(ctl[2], nsteps)
    return None


@pytest.mark.parametrize("case", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_step_local_parity(case):
    import ocplasma_amd as oc
    c = case
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    a = _make(oc, c)
    b = _make(oc, c)
    c.dt = a.dt                      # after the CFL clamp (pic.py:71-73)
    try:
        va, vb = a.torch_views(), b.torch_views()
        if c.sampled:
            a.reset_sampled("bump-on-tail", seed=9)
            b.reset_sampled("bump-on-tail", seed=9)
        else:
            x0, v0 = _initial_state(c, rng)
            for env in (a, b):
                if c.planted == "far_set":
                    env._h.set_particles(x0, v0)
                    env.refresh()
                else:
                    env.reset(x0, v0)
            _check_loaded(c, a, x0, va)
        ctl, E_host, ext_err = _controls(oc, c, rng, c.envs)
        if ctl is not None and ctl[0] == "act":
            a.set_actuator(ctl[1])
            b.set_actuator(ctl[1])
        tag = repr(c)
        states = {e: [_read(a, c, e, va)] for e in range(c.check_envs)}
        for e in range(c.check_envs):
            check_stages(c, states[e][0], tag + f" env {e} loaded")
        for k in range(c.steps):
            _step(a, ctl)
            for e in range(c.check_envs):
                post = _read(a, c, e, va)
                t = tag + f" env {e} step {k + 1}"
                check_stages(c, post, t)
                check_push(c, states[e][-1], post, None if E_host is None else E_host[e], ext_err, t)
                states[e].append(post)
        assert a.bad_count() == 0, tag
        # the twin: the same steps in ONE call, energies of every inner step recorded
        if ctl is not None and ctl[0] == "act":
            hist = b.step_actions_traj(np.repeat(ctl[2][None], c.steps, axis=0), history=True)
        else:
            hist = b.step_history(None if ctl is None else ctl[1], c.steps)
        ke, pe, per = hist
        for e in range(c.check_envs):
            for k in range(c.steps):
                st = states[e][k + 1]
                check_energies_of(c, st["x"], st["v"], ke[k, e], pe[k, e], per[k, e], tag + f" multi-step env {e} step {k + 1}")
            fin = _read(b, c, e, vb)
            # one call of k steps and k calls of one step: the same state bit for bit (the check_push below takes its
            # pre-state from the single-stepping handle).  Not for the float64 accumulator: its running sums (ds_add_f64) are
            # order-dependent in the last bits by design (csrc/pic_device.h, LDS accumulators), so two runs may differ there; the derived bounds still hold
            last = states[e][-1]
            if _acc_kind(c) != "float64":
                for key in ("x", "v", "n", "E_mesh", "phi"):
                    assert np.array_equal(fin[key].view(np.uint8), last[key].view(np.uint8)), (tag, "multi-step vs single steps", e, key)
            check_stages(c, fin, tag + f" multi-step env {e} final")
            check_push(c, states[e][-2], fin, None if E_host is None else E_host[e], ext_err, tag + f" multi-step env {e} final")
        assert b.bad_count() == 0, tag
    finally:
        a.close()
        b.close()


def test_fixed32_displacements_of_half_a_box_are_counted_as_bad():
    """pic_device.h:372-390: a fixed-point drift of half a box or more per sub-stage is not representable and is counted; the
    other particles are not.  The counter counts drift evaluations, a fixed number per step for each schedule.  With
    |c1 v dt| = 0.7 L the c1 and c4 drifts are unrepresentable and the c2 = c3 ones (0.26 of it) are not, so per planted
    particle:
      the refresh of a reset:  1  (the next step's q1, deposited ahead)
      a resident step:         4  (q1 of the deposit that opens the launch, q1 again in the kick phase, c4, the next q1)
      a streaming step:        3  (sweep A is skipped, its deposit was made by the refresh: sweep B's q1, sweep D's c4 and
                                   next q1)
    and nothing for any other particle."""
    import ocplasma_amd as oc
    N, Ng, L, dt = 4096, 64, 10.0, 0.05
    rng = np.random.default_rng(7)
    cs, _ = hp.yoshida4_coefficients()
    c1 = float(cs[0])
    x0 = rng.uniform(0, L, (1, N)).astype(np.float32)
    v0 = rng.normal(0, 1, (1, N)).astype(np.float32)
    for bpe, per_step in ((-1, 4), (2, 3)):
        env = oc.BatchedPIC(1, N, Ng, L=L, dt=dt, dtype="float32", position_dtype="fixed32", blocks_per_env=bpe)
        try:
            assert env._h.schedule() == ("resident" if bpe == -1 else "streaming")
            env.reset(x0, v0)
            env.step(None, 1)
            assert env.bad_count() == 0
            fast = v0.copy()
            k = 5
            fast[0, :k] = 0.7 * L / (c1 * dt) * np.where(np.arange(k) % 2, 1.0, -1.0)
            env.reset(x0, fast)
            at_reset = env.bad_count()
            env.step(None, 1)
            grown = env.bad_count() - at_reset
            record_measure(f"fixed32_bad_count_per_fast_particle_reset_bpe{bpe}", at_reset / k)
            record_measure(f"fixed32_bad_count_per_fast_particle_step_bpe{bpe}", grown / k)
            assert at_reset == k and grown == per_step * k, (bpe, at_reset, grown)
        finally:
            env.close()


def test_accumulator_rounds_to_nearest():
    """Exact weights, known sums: L = Ng = 64 (dx = 1), float64 CIC, positions j + f with f = (k + 3/4) 2^-fg + 1/2 whose
    weights are exact in float64 and lie a quarter unit off the 2^-fg grid.  The 64-bit accumulator must hold the
    round-to-nearest sums exactly; the density is (double)acc 2^-fg times the host's scale, two float64 roundings."""
    import ocplasma_amd as oc
    N, Ng, L = 1 << 20, 64, 64.0
    fg = _fg(N)
    rng = np.random.default_rng(3)
    j = rng.integers(0, Ng, N)
    kk = rng.integers(0, 1 << 8, N)
    num = (kk.astype(object) * 4 + 3)                          # f = 1/2 + num 2^-(fg+2)
    f = 0.5 + np.array([float(t) for t in num]) * 2.0 ** -(fg + 2)
    x = j.astype(np.float64) + f
    assert np.all(x - j == f)                                 # exact in float64
    # integer weights in units of 2^-(fg+2): wr = 2^(fg+1) + num, wl = 2^(fg+2) - wr; rounded to 2^-fg (nearest)
    wr4 = (1 << (fg + 1)) + num
    wl4 = (1 << (fg + 2)) - wr4
    rnd = lambda t: (t + 2) // 4                              # noqa: E731  (t = 4 a + 1 or 4 a + 3: never a tie)
    acc = [0] * Ng
    for jj, a_, b_ in zip(j.tolist(), wl4.tolist(), wr4.tolist()):
        acc[jj] += rnd(a_)
        acc[(jj + 1) % Ng] += rnd(b_)
    scale = 1.0 * L / N / (L / Ng)
    want = np.array([float(t) * 2.0 ** -fg * scale for t in acc])
    env = oc.BatchedPIC(1, N, Ng, L=L, dt=0.01, dtype="float64", accum_dtype="fix64")
    try:
        env.reset(x[None], np.zeros((1, N)))
        n = env.fields()[0][0]
    finally:
        env.close()
    err = np.max(np.abs(n - want) / np.abs(want))
    record_measure("accumulator_exact_rel", err)
    assert err <= 2 * U64, err


@pytest.mark.parametrize("dtype,pos", [("float32", "float"), ("float32", "fixed32"), ("float64", "float")])
def test_phase_histogram_edges(dtype, pos):
    """phase_hist_kernel against np.histogram2d of the exact positions, with positions and velocities on every bin edge and
    one ulp to either side, random nbins and [vmin, vmax]."""
    import ocplasma_amd as oc
    rng = np.random.default_rng(zlib.crc32((dtype + pos).encode()))
    L = float(rng.choice([1.0, 10.0, 50.0]))
    for _ in range(3):
        nb = int(rng.integers(2, 40))
        vmin = float(rng.uniform(-8, -1))
        vmax = float(rng.uniform(1, 8))
        W = np.dtype(dtype).type
        xe = (np.arange(nb) * W(L / nb)).astype(dtype)
        ve = (W(vmin) + np.arange(nb + 1) * W((vmax - vmin) / nb)).astype(dtype)
        xs = np.concatenate([xe, np.nextafter(xe, W(-1)), np.nextafter(xe, W(2 * L)), rng.uniform(0, L, 64).astype(dtype)])
        vs = np.concatenate([ve, np.nextafter(ve, W(-100)), np.nextafter(ve, W(100)), rng.uniform(vmin - 1, vmax + 1, 64).astype(dtype)])
        N = max(xs.size, vs.size)
        xs = np.resize(xs, N)
        vs = np.resize(vs, N)
        rng.shuffle(vs)
        env = oc.BatchedPIC(1, N, 16, L=L, dt=0.01, dtype=dtype, position_dtype=pos)
        try:
            env.reset(xs[None], vs[None])
            views = env.torch_views()
            env.sync()
            if pos == "fixed32":
                xd = hp.fixed_to_length(views["x_fixed"][0].cpu().numpy().view(np.uint32), L)
            else:
                xd = hp.as_ld(views["x"][0].cpu().numpy())
            vd = views["v"][0].cpu().numpy().astype(np.float64)
            counts = env._h.phase_histogram(nb, vmin, vmax)[0]
        finally:
            env.close()
        # estimate_f (objective.py:8-14): np.histogram2d over [[0, L], [vmin, vmax]]
        want, _, _ = np.histogram2d(xd.astype(np.float64), vd, bins=[nb, nb], range=[[0, L], [vmin, vmax]])
        assert np.array_equal(counts, want.astype(counts.dtype)), (dtype, pos, nb, vmin, vmax)


@pytest.mark.parametrize("Ng,bpe", [(4, 0), (17, 0), (64, -1), (64, 2), (1024, 0), (2722, 2)])
def test_modes_and_feedback_against_longdouble_dft(Ng, bpe):
    import ocplasma_amd as oc
    N, L = 4000, 50.0
    rng = np.random.default_rng(Ng)
    x0 = rng.uniform(0, L, (2, N))
    v0 = rng.normal(0, 1, (2, N))
    for M in sorted({1, min(16, Ng - 1)}):
        env = oc.BatchedPIC(2, N, Ng, L=L, dt=0.05, blocks_per_env=bpe)
        try:
            if bpe:
                assert env._h.schedule() == ("resident" if bpe == -1 else "streaming")
            env.reset(x0, v0)
            E = env.fields()[1]
            ek = env.modes(M)
            for e in range(2):
                re, im = hp.modes(E[e], M)
                # sum of Ng products with float64 twiddles (each off by u64) over a workgroup, then / Ng * 2
                b = (Ng / 512 + 20) * U64 * 2 * float(np.sum(np.abs(E[e]))) / Ng + U64 * float(np.max(np.abs(E[e])))
                err = max(float(np.max(np.abs(ek[e].real - re))), float(np.max(np.abs(ek[e].imag - im))))
                assert err <= b, (Ng, M, err, b)
                _ratio("modes", err, b)
            # the feedback law on the device, on both schedules' step functions: the action of each step from the E_mesh
            # before it (single-step calls, so that fields() shows that E_mesh)
            act = oc.E_field(L, Ng, M)
            env.set_actuator(act)
            for _ in range(2):
                E = env.fields()[1]
                got = env.step_feedback(1, actions=True)["actions"][0]
                for e in range(2):
                    want = hp.feedback_action(E[e], M)
                    b = (Ng / 512 + 20) * U64 * 2 * float(np.sum(np.abs(E[e]))) / Ng + U64 * float(np.max(np.abs(E[e])))
                    err = float(np.max(np.abs(got[e] - want)))
                    assert err <= b, (Ng, M, err, b)
                    _ratio("feedback", err, b)
        finally:
            env.close()
