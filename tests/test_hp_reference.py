"""Pins tests/hp_reference.py (the extended-precision comparator of tests/test_gpu_local_parity.py) to the reference wherever
the reference is defined: the golden vectors it produced, an FFT solve of the same stencil, and the NumPy oracle's step.
CPU only."""
import numpy as np
import pytest

import hp_reference as hp
from conftest import circ_err, load_golden, rel_err
from oracle import pic_oracle as po

LD = hp.LD


def test_longdouble_is_extended():
    assert np.finfo(hp.LD).eps < 1e-18
    assert hp.deposit(np.array([0.3]), 4, 1.0, 1.0, 1)[0].dtype == hp.LD


def test_g1_deposit():
    """CIC and TSC densities of the golden positions (raw, outside the box included: wrapped as the reference wraps them)."""
    g = load_golden("g1_deposit")
    L, Ng, n0 = float(g["L"]), int(g["Ng"]), float(g["n0"])
    x = g["x"][:, 0]
    N = x.size
    n, count = hp.deposit(x, Ng, L, n0, N, "CIC")
    # the reference sums float64 weights with bincount: its own error is a few ulps of the node sums
    assert rel_err(n.astype(float), g["n"]) < 1e-14
    assert count.sum() == 2 * N
    n, count = hp.deposit(x, Ng, L, n0, N, "TSC")
    assert rel_err(n.astype(float), g["tsc_n"]) < 1e-14
    assert count.sum() == 3 * N
    xin = g["xin"][:, 0]
    assert rel_err(hp.deposit(xin, Ng, L, n0, 500, "CIC")[0].astype(float), g["n_d"]) < 1e-14


@pytest.mark.parametrize("Ng", [128, 250, 256, 1024])
def test_g2_solve(Ng):
    """E_mesh and the mean-removed potential of the reference's Sherman-Morrison solve (whose gauge depends on gamma)."""
    g = load_golden("g2_solve")
    L, n0 = float(g["L"]), float(g["n0"])
    E, phi = hp.solve(g[f"n_{Ng}"], n0, L)
    # the reference's two gammas disagree with each other by up to 1e-11 (test_oracle_golden.test_g2_field_is_gauge_free)
    for gamma in ("5.0", "0.3"):
        assert rel_err(E.astype(float), g[f"E_{Ng}_g{gamma}"]) < 2e-11
        ref = g[f"phi_{Ng}_g{gamma}"]
        assert rel_err(phi.astype(float), ref - ref.mean()) < 2e-11


def test_g3_compute_E():
    g = load_golden("g3_compute_E")
    L, Ng, n0 = float(g["L"]), int(g["Ng"]), float(g["n0"])
    x = g["x"][:, 0]
    N = x.size
    n, _ = hp.deposit(x, Ng, L, n0, N, "CIC")
    E, phi = hp.solve(n, n0, L)
    assert rel_err(E.astype(float), g["E_mesh"]) < 1e-12
    assert rel_err(hp.gather(E, x, L, "CIC").astype(float), g["E"]) < 1e-12
    ext = g["E_ext"][:, 0]
    assert rel_err((E + ext).astype(float), g["E_mesh_with_ext"]) < 1e-12
    assert rel_err(hp.gather(E + ext, x, L, "CIC").astype(float), g["E_with_ext"]) < 1e-12
    nt, _ = hp.deposit(x, Ng, L, n0, N, "TSC")
    Et = hp.solve(nt, n0, L)[0] + ext
    assert rel_err(Et.astype(float), g["tsc_E_mesh_with_ext"]) < 1e-12
    assert rel_err(hp.gather(Et, x, L, "TSC").astype(float), g["tsc_E_with_ext"]) < 1e-12
    ke, pe, per = hp.energies(np.zeros(N), E, L, N)
    assert ke == 0 and abs(float(pe) / float(g["PE"]) - 1) < 1e-12


@pytest.mark.parametrize("name,shape,ext", [("g4_bump_on_tail_ext_N4000_Ng256", "CIC", True),
                                             ("g4_tsc_bump_on_tail_ext_N3000_Ng128", "TSC", True),
                                             ("g5_two_stream_N5000_Ng250", "CIC", False),
                                             ("g5_bump_on_tail_N10000_Ng128", "CIC", False)])
def test_first_step_of_the_golden_trajectories(name, shape, ext):
    g = load_golden(name)
    L, Ng, n0, N, dt = float(g["L"]), int(g["Ng"]), float(g["n0"]), int(g["N"]), float(g["dt"])
    E_ext = None
    if ext:
        mm = g["actions"].shape[1] // 2
        a = g["actions"][0]
        E_ext = po.actuator_field(L, Ng, mm, a[:mm], a[mm:])[:, 0]
    x, v, _ = hp.yoshida4_step(g["x_init"][:, 0], g["v_init"][:, 0], E_ext, dt, Ng, L, n0, N, shape, np.float64)
    # the reference's own step carries float64 rounding of the positions (|x| <= L) and velocities
    assert circ_err(x.astype(float), g["x_1"], L) / L < 1e-13
    assert np.max(np.abs(v.astype(float) - g["v_1"][:, 0])) / np.max(np.abs(g["v_1"])) < 1e-13
    n, _ = hp.deposit(x, Ng, L, n0, N, shape)
    assert rel_err(n.astype(float), g["n_1"]) < 1e-12
    E, phi = hp.solve(n, n0, L)          # the post-step field has no external part (pic.py:145-146)
    assert rel_err(E.astype(float), g["E_mesh_1"]) < 1e-11
    ref = g["phi_mesh_1"][:, 0]
    assert rel_err(phi.astype(float), ref - ref.mean()) < 1e-11


def _fft_solve(b, L):
    """float64 spectral solve of the same 3-point stencil: eigenvalues -4/dx^2 sin^2(pi k / Ng), k = 0 dropped."""
    Ng = b.size
    dx = L / Ng
    bk = np.fft.fft(b)
    lam = -4.0 / dx ** 2 * np.sin(np.pi * np.arange(Ng) / Ng) ** 2
    pk = np.zeros_like(bk)
    pk[1:] = bk[1:] / lam[1:]
    phi = np.fft.ifft(pk).real
    E = -(np.roll(phi, -1) - np.roll(phi, 1)) / (2 * dx)
    return E, phi


@pytest.mark.parametrize("L", [1.0, 10.0, 50.0, 77.7])
def test_solve_agrees_with_a_spectral_solve(L):
    """Mesh sizes over 4..3267, the sizes at which the reference's Sherman-Morrison solve is singular included (100 and 300
    at L = 50, the largest meshes 2722 and 3267)."""
    rng = np.random.default_rng(int(L * 10))
    sizes = sorted(set([4, 5, 63, 64, 65, 100, 127, 128, 129, 300, 511, 512, 513, 1023, 1024, 1025, 1159, 1249, 2039,
                        2722, 3267] + [int(s) for s in rng.integers(4, 3268, 12)]))
    for Ng in sizes:
        N = 20 * Ng
        n, _ = hp.deposit(rng.uniform(0, L, N), Ng, L, 1.0, N, "CIC")
        E, phi = hp.solve(n, 1.0, L)
        b = (n - LD(1.0)).astype(float)
        b -= b.mean()
        Ef, pf = _fft_solve(b, L)
        # float64 FFT error: a few ulps times log2(Ng) of the largest values; the longdouble solve is ~1e-19
        tol = 1e-13 * max(1.0, np.log2(Ng))
        assert rel_err(E.astype(float), Ef) < tol, Ng
        assert rel_err(phi.astype(float), pf - pf.mean()) < tol, Ng
        # the discrete equation itself, in longdouble
        dx = LD(L) / LD(Ng)
        lap = (np.roll(phi, -1) - 2 * phi + np.roll(phi, 1)) / dx ** 2
        assert np.max(np.abs(lap - (n - np.mean(n)))) < 1e-14 * max(1.0, float(np.max(np.abs(n)))), Ng


@pytest.mark.parametrize("shape", ["CIC", "TSC"])
def test_one_step_agrees_with_the_oracle(shape):
    rng = np.random.default_rng(11 if shape == "CIC" else 12)
    compared = 0
    for _ in range(30):
        N = int(rng.choice([1, 3, 64, 257, 2049]))
        Ng = int(rng.choice([4, 5, 16, 64, 100, 127, 250]))
        L = float(rng.choice([1.0, 10.0, 50.0, 77.7]))
        n0 = float(rng.choice([0.5, 1.0]))
        dt = float(rng.choice([0.01, 0.1]))
        x0 = rng.uniform(-0.25 * L, 1.25 * L, N)
        v0 = rng.normal(0, 1, N)
        E_ext = rng.uniform(-0.5, 0.5, Ng) if rng.integers(0, 2) else None
        try:
            with np.errstate(all="ignore"):
                ref = po.OraclePIC(x0, v0, Ng, n0=n0, L=L, dt=dt, interpol=shape, perturb=False, faithful=False)
                xr, vr = ref._lean_step(None if E_ext is None else E_ext.reshape(-1, 1))
        except ValueError:                             # NaN positions reach np.bincount, as they would in the reference
            continue
        if not (np.isfinite(xr).all() and np.isfinite(vr).all() and np.isfinite(ref.E_mesh).all()):
            continue                                   # the reference's solve is singular at this (L, Ng)
        x, v, _ = hp.yoshida4_step(x0, v0, E_ext, ref.dt, Ng, L, n0, N, shape, np.float64)
        tag = (N, Ng, L, n0, dt, shape)
        assert circ_err(x.astype(float), np.mod(xr, L), L) / L < 1e-12, tag
        assert np.max(np.abs(v.astype(float) - vr[:, 0])) / max(1.0, np.max(np.abs(vr))) < 1e-12, tag
        compared += 1
    assert compared >= 8


def test_fixed_point_cells_are_exact():
    """uint32 positions: cell and offset from integer arithmetic, also on the cell edges u = k 2^32 / Ng."""
    Ng, L = 64, 50.0
    u = np.array([0, 1, 2 ** 26, 2 ** 26 - 1, 2 ** 32 - 1, 3 * 2 ** 26], dtype=np.uint32)
    jf, d = hp._cells(u, Ng, L)
    assert list(jf) == [0, 0, 1, 0, 63, 3]
    assert d[0] == 0 and d[2] == 0 and d[5] == 0 and 0 < d[1] < 1e-7 and 1 - d[3] < 1e-7
    n, count = hp.deposit(u, Ng, L, 1.0, u.size, "CIC")
    assert abs(float(np.sum(n)) * (L / Ng) - L) < 1e-15 * L


def test_modes_match_fft():
    rng = np.random.default_rng(5)
    for Ng in (4, 17, 64, 1024, 2722):
        E = rng.normal(size=Ng)
        M = min(16, Ng - 1)
        re, im = hp.modes(E, M)
        ref = (np.fft.fft(E) / Ng * 2.0)[1:M + 1]
        assert np.max(np.abs(re.astype(float) - ref.real)) < 1e-14 * max(1, np.log2(Ng)), Ng
        assert np.max(np.abs(im.astype(float) - ref.imag)) < 1e-14 * max(1, np.log2(Ng)), Ng
        a = hp.feedback_action(E, M)
        assert np.array_equal(a[:M], -re) and np.array_equal(a[M:], im)
