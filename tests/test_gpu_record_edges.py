"""The rollout recorder (csrc/pic_record.h: record_hist_kernel, record_finish_kernel; planned by csrc/host_blocks.h: record_plan) at
its bin, LDS-layout and launch-geometry edges: the cases, data, references and bounds of tests/hp_record.py, through the public
methods of BatchedPIC.  Every case asserts the plan values it is named for through hp_record.plan (pinned against the C++ by
tests/test_record_edges_cpu.py).  Histograms and `inside` equal NumPy's on the float64 image of the particles the device holds;
entropy and KL lie within hp_record.sum_bound of the longdouble value from the exact counts; spectrum rows and field energy
within their bounds.  Phase-space counts are no part of a record: the entropy pins their multiset, the KL against a target
without zero bins where each sits (hp_record.py).  The worst err / bound of every group is recorded under record_edges.<group>
and listed in profiles/record_edges.md."""
import numpy as np
import pytest

import hp_record as hr
from conftest import record_measure

pytestmark = pytest.mark.gpu

_WORST = {}


def _ratio(group, err, bound):
    err, bound = float(err), float(bound)
    r = 0.0 if err == 0 else (err / bound if bound > 0 else np.inf)
    _WORST[group] = max(_WORST.get(group, 0.0), r)
    record_measure(f"record_edges.{group}", _WORST[group])
    return r


def _new(c, Ng=16, n0=1.0):
    from ocplasma_amd.env.batched import BatchedPIC
    dtype, pos, vec = hr.FORMATS[c.fmt]
    p = hr.plan(c.N, vec, c.E, c.xb, c.vb, c.px, c.pv)
    assert {k: p[k] for k in c.claim} == c.claim, (c.name, p)             # the case runs the path it is named for
    return BatchedPIC(c.E, c.N, Ng, n0=n0, L=hr.L, dt=0.1, dtype=dtype, position_dtype=pos)


def _held(env):
    """(x, v) [E, N]: the float64 image of the particles the device holds (fixed-point positions as pos_to_length has them)."""
    env.sync()
    t = env.torch_views()
    if env.fixed_positions:
        x = (t["x_fixed"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.float64) * (env.L * 2.0 ** -32)
    else:
        x = t["x"].cpu().numpy().astype(np.float64)
    return x, t["v"].cpu().numpy().astype(np.float64)


def _start(env, c, M=0, feq=None, **kw):
    env.start_recording(modes=M, x_bins=c.xb, v_bins=c.vb, phase_bins=(c.px, c.pv) if c.px else None, vmin=hr.VMIN, vmax=hr.VMAX,
                        feq=feq, **kw)


def _check_counts(name, rec, r, e, ref):
    for key in ("x_hist", "v_hist"):
        got = getattr(rec, key)[r, e]
        bad = np.flatnonzero(got != ref[key])
        assert got.shape == ref[key].shape and bad.size == 0, (name, key, r, e, bad[:8], got[bad[:8]], ref[key][bad[:8]])
    assert rec.inside[r, e] == ref["inside"], (name, r, e, rec.inside[r, e], ref["inside"])


def _check_sums(group, name, rec, r, e, phase, n0, pdx, pdv, N, feq):
    want = hr.entropy_kl(phase, n0, pdx, pdv, N, feq)
    for key, got, w, T in (("entropy", rec.entropy[r, e], want["S"], want["T_S"]), ("kl", rec.kl[r, e], want["KL"], want["T_KL"])):
        if w is None:
            assert np.isnan(got), (name, key, got)
            continue
        b = hr.sum_bound(phase.size, T, want["F"], pdx, pdv)
        err = abs(hr.LD(got) - w)
        ratio = _ratio(f"{group}.{key}", err, b)
        print(f"{name} record {r} env {e} {key}: device {got!r} err {float(err):.3e} bound {b:.3e} ratio {ratio:.3f}")
        assert np.isfinite(got) and err <= b, (name, key, r, e, got, float(w), float(err), b)


def _check_mesh(group, name, rec, r, e, E_mesh, dx):
    M = rec.Ek.shape[2]
    re, im = hr.rows(E_mesh, M)
    b = hr.rows_bound(E_mesh)
    err = max([float(np.max(np.abs(rec.Ek[r, e].real - re))), float(np.max(np.abs(rec.Ek[r, e].imag - im)))]) if M else 0.0
    bf = hr.field_energy_bound(E_mesh, dx)
    ef = abs(hr.LD(rec.field_energy[r, e]) - hr.field_energy(E_mesh, dx))
    print(f"{name} record {r} env {e} M {M}: rows err {err:.3e} bound {b:.3e}; field energy err {float(ef):.3e} bound {bf:.3e}")
    _ratio(f"{group}.rows", err, b)
    _ratio(f"{group}.field_energy", ef, bf)
    assert err <= b and ef <= bf, (name, r, e, M, err, b, float(ef), bf)
    if M:
        assert rec.Ek[r, e, 0].imag == 0


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _run_static(group, name):
    """One case on a state loaded by reset (or set_particles) and never stepped: record_now under a target with zero bins and
    under one without (the phase group; the others take the first), every environment against NumPy on the particles it holds."""
    c = hr.CASES[name]
    env = _new(c)
    X, V = hr.case_data(c)
    if c.load == "reset":
        env.reset(X, V)
    else:
        env._h.set_particles(X, V)
    x, v = _held(env)
    if not env.fixed_positions:      # the edges have reached the device: reset folds positions outside [0, L), nothing else moves
        keep = (X >= 0) & (X < hr.L) if c.load == "reset" else np.ones(X.shape, dtype=bool)
        assert np.array_equal(x[keep], X.astype(np.float64)[keep])
    assert np.array_equal(v, V.astype(np.float64), equal_nan=True)
    distinct = min(c.E, 3)
    assert all(np.array_equal(x[e], x[e % 3]) and np.array_equal(v[e], v[e % 3], equal_nan=True) for e in range(distinct, c.E))
    refs = [hr.counts(x[e], v[e], hr.L, c.xb, c.vb, c.px, c.pv, hr.VMIN, hr.VMAX) for e in range(distinct)]
    if c.E == 2:
        assert all(np.array_equal(refs[0][k], refs[1][k]) for k in ("x_hist", "v_hist", "phase", "inside"))
    targets = [None]
    if c.px:
        targets = [hr.target(c.px, c.pv, 5)] + ([hr.target(c.px, c.pv, 6, zeros=False)] if group == "phase" else [])
    scalars = c.load == "reset" and not c.nonfinite
    for feq in targets:
        _start(env, c, M=2 if scalars else 0, feq=feq)
        env.record_now()
        rec = env.recorded()
        env.stop_recording()
        assert np.array_equal(rec.steps, [0]) and rec.x_hist.shape == (1, c.E, c.xb) and rec.v_hist.shape == (1, c.E, c.vb)
        for e in range(c.E):
            ref = refs[e % 3]
            _check_counts(name, rec, 0, e, ref)
            if c.nonfinite:
                continue                 # (only the histograms and `inside` of a state with non-finite velocities)
            if c.px and e < distinct:
                _check_sums(group, name, rec, 0, e, ref["phase"], 1.0, *hr.phase_steps(hr.L, c.px, c.pv, hr.VMIN, hr.VMAX), c.N, feq)
            elif not c.px:
                assert np.isnan(rec.entropy[0, e]) and np.isnan(rec.kl[0, e])
            # environments with the same particles, in any order, agree bit for bit
            first = 0 if c.E == 2 else e % 3
            assert _same_bits(rec.entropy[0, e], rec.entropy[0, first]) and _same_bits(rec.kl[0, e], rec.kl[0, first]), (name, e)
        if scalars:
            ke, pe, per = env.energies()
            assert _same_bits(rec.KE[0], ke) and _same_bits(rec.PE[0], pe) and _same_bits(rec.PE_reward[0], per)
            E_mesh = env.fields()[1]
            for e in range(distinct):
                _check_mesh(group, name, rec, 0, e, E_mesh[e], env.dx)
    env.close()


# ---- 1. data on the bin edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in hr.GROUPS["edges"]])
def test_bin_edges(name):
    _run_static("edges", name)


# ---- 2. copies per marginal bin ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in hr.GROUPS["copies"]])
def test_copies_per_marginal_bin(name):
    _run_static("copies", name)


# ---- 3. the phase histogram in LDS and in global memory -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in hr.GROUPS["phase"]])
def test_phase_placement(name):
    _run_static("phase", name)


# ---- 4. the particle tail and the launch geometry -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in hr.GROUPS["tails"]])
def test_tails_and_geometry(name):
    _run_static("tails", name)


# ---- 5. several records ------------------------------------------------------------------------------------------------------------------
_RECORD_FIELDS = ("steps", "KE", "PE", "PE_reward", "field_energy", "entropy", "kl", "inside", "Ek", "x_hist", "v_hist")


@pytest.mark.parametrize("fmt", list(hr.FORMATS))
@pytest.mark.parametrize("tag", list(hr.MULTI))
def test_several_records(fmt, tag):
    """step(nsteps=3) at stride 1 against three single-step calls with the particles read in between: the same bits, and each
    record is of its own step's particles.  Then another recording with other bin counts on the same handle."""
    c, c2 = hr.CASES[f"multi-{fmt}-{tag}"], hr.CASES[f"multi-{fmt}-{tag}-restart"]
    a, b = _new(c), _new(c)
    feq = hr.target(c.px, c.pv, 5)
    for env in (a, b):
        env.reset_sampled(seed=13)
        _start(env, c, M=3, feq=feq, stride=1)
    a.step(nsteps=3)
    held, meshes = [], []
    for _ in range(3):
        b.step()
        held.append(_held(b))
        meshes.append(b.fields()[1])
    ra, rb = a.recorded(), b.recorded()
    a.close()
    assert np.array_equal(rb.steps, [1, 2, 3])
    for k in _RECORD_FIELDS:
        assert _same_bits(getattr(ra, k), getattr(rb, k)), (fmt, tag, k)

    def check(name, case, rec, r, state, E_mesh, target):
        x, v = state
        for e in range(case.E):
            ref = hr.counts(x[e], v[e], hr.L, case.xb, case.vb, case.px, case.pv, hr.VMIN, hr.VMAX)
            _check_counts(name, rec, r, e, ref)
            _check_sums("multi", name, rec, r, e, ref["phase"], 1.0, *hr.phase_steps(hr.L, case.px, case.pv, hr.VMIN, hr.VMAX), case.N, target)
            _check_mesh("multi", name, rec, r, e, E_mesh[e], b.dx)
    for r in range(3):
        check(c.name, c, rb, r, held[r], meshes[r], feq)
    assert not _same_bits(rb.x_hist[0], rb.x_hist[2])                       # (the particles have moved)
    b.stop_recording()
    feq2 = hr.target(c2.px, c2.pv, 8)
    p2 = hr.case_plan(c2)
    assert {k: p2[k] for k in c2.claim} == c2.claim
    _start(b, c2, M=3, feq=feq2, stride=1)
    b.record_now()
    b.step()
    rec = b.recorded()
    assert np.array_equal(rec.steps, [0, 1])
    check(c2.name, c2, rec, 0, held[2], meshes[2], feq2)
    check(c2.name, c2, rec, 1, _held(b), b.fields()[1], feq2)
    b.close()


# ---- 6. the finishing kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ng", hr.FINISH_MESHES)
def test_spectrum_rows_and_field_energy(Ng):
    from ocplasma_amd.env.batched import BatchedPIC
    Ms = hr.finish_modes(Ng)
    env = BatchedPIC(2, hr.N_ODD, Ng, L=hr.L, dt=0.1)
    env.reset_sampled(seed=Ng)
    env.start_recording(stride=2, modes=Ms[-1])            # up to the Nyquist row, recorded by the second step itself
    env.step(nsteps=2)
    recs = [env.recorded()]
    env.stop_recording()
    for M in Ms[:-1]:
        env.start_recording(modes=M)
        env.record_now()
        recs.append(env.recorded())
        env.stop_recording()
    E_mesh = env.fields()[1]
    ke, pe, per = env.energies()
    env.close()
    assert np.array_equal(recs[0].steps, [2])
    for rec, M in zip(recs, [Ms[-1]] + Ms[:-1]):
        assert rec.Ek.shape == (1, 2, M) and rec.ks.shape == (M,)
        assert _same_bits(rec.KE[0], ke) and _same_bits(rec.PE[0], pe) and _same_bits(rec.PE_reward[0], per)
        assert np.isnan(rec.entropy).all() and np.isnan(rec.kl).all() and np.array_equal(rec.inside, [[hr.N_ODD] * 2])
        for e in range(2):
            _check_mesh("finish", f"Ng{Ng}", rec, 0, e, E_mesh[e], hr.L / Ng)
        # the rows a shorter record shares with the longest are the same bits
        assert _same_bits(rec.Ek[0, :, :M], recs[0].Ek[0, :, :M]) and _same_bits(rec.field_energy, recs[0].field_energy)


@pytest.mark.parametrize("name", list(hr.FINISH_SCALARS))
def test_finishing_scalars(name):
    from ocplasma_amd.env.batched import BatchedPIC
    n0, vmin, vmax, phase_dx, phase_dv, kind = hr.FINISH_SCALARS[name]
    nb = hr.FINISH_BINS
    X, V = hr.finish_data(kind, hr.N_ODD, 7)
    env = BatchedPIC(2, hr.N_ODD, 16, n0=n0, L=hr.L, dt=0.1)
    env.reset(X, V)
    feq = hr.target(nb, nb, 5)
    env.start_recording(modes=0, x_bins=nb, v_bins=nb, phase_bins=nb, vmin=vmin, vmax=vmax, feq=feq, phase_dx=phase_dx, phase_dv=phase_dv)
    env.record_now()
    rec = env.recorded()
    x, v = _held(env)
    env.close()
    pdx, pdv = hr.phase_steps(hr.L, nb, nb, vmin, vmax, phase_dx, phase_dv)
    for e in range(2):
        ref = hr.counts(x[e], v[e], hr.L, nb, nb, nb, nb, vmin, vmax)
        _check_counts(name, rec, 0, e, ref)
        _check_sums("finish", name, rec, 0, e, ref["phase"], n0, pdx, pdv, hr.N_ODD, feq)
    assert _same_bits(rec.entropy[0, 0], rec.entropy[0, 1]) and _same_bits(rec.kl[0, 0], rec.kl[0, 1])
    if name == "empty-window":
        assert not rec.inside.any() and not rec.v_hist.any() and (rec.entropy == 0).all() and (rec.kl == 0).all()
        assert (rec.x_hist.sum(axis=2) == hr.N_ODD).all()
    if name == "one-bin":
        assert (rec.inside == hr.N_ODD).all() and (rec.x_hist.max(axis=2) == hr.N_ODD).all() and (rec.v_hist.max(axis=2) == hr.N_ODD).all()


# ---- 7. the twiddle table grows under a running recorder -----------------------------------------------------------------------------------
def test_twiddle_table_regrown_by_modes():
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(2, hr.N_ODD, 64, L=hr.L, dt=0.1)
    env.reset_sampled(seed=4)
    env.step(nsteps=2)
    env.start_recording(modes=3)                 # two twiddle rows
    env.record_now()
    env.modes(12)                                # twelve: the sine block moves
    env.record_now()
    rec = env.recorded()
    E_mesh = env.fields()[1]
    env.close()
    assert _same_bits(rec.Ek[0], rec.Ek[1]) and _same_bits(rec.field_energy[0], rec.field_energy[1])
    for e in range(2):
        _check_mesh("twiddle", "modes", rec, 1, e, E_mesh[e], hr.L / 64)


def test_twiddle_table_regrown_by_an_actuator():
    """A handle whose table grows inside a feedback step, under the recorder, against one that grew it before recording."""
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    recs = []
    for grown_first in (False, True):
        env = BatchedPIC(2, hr.N_ODD, 64, L=hr.L, dt=0.1)
        env.reset_sampled(seed=4)
        act = oc.E_field(hr.L, 64, 12)
        if grown_first:
            env.set_actuator(act)
            env.modes(12)
        env.start_recording(stride=1, modes=3)
        env.record_now()
        if not grown_first:
            env.set_actuator(act)
        env.step_feedback(1)
        env.record_now()
        recs.append(env.recorded())
        E_mesh = env.fields()[1]
        env.close()
    a, b = recs
    assert np.array_equal(a.steps, [0, 1, 1])
    for k in _RECORD_FIELDS:
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    assert _same_bits(a.Ek[1], a.Ek[2]) and not _same_bits(a.Ek[0], a.Ek[1])
    for e in range(2):
        _check_mesh("twiddle", "actuator", a, 2, e, E_mesh[e], hr.L / 64)
