"""The field probes -- pic_eval_field, pic_compute_E, pic_gather_E, pic_get_cic, pic_solve_poisson -- against
tests/hp_reference.py (longdouble), with the bounds of tests/hp_checks.py, for every particle format, shape, accumulator and a
spread of (N, Ng, L).

The reference positions are what the device holds: for float formats the input in the particle dtype wrapped by
np.mod(np.mod(x, L), L) in that dtype (what the device's wrap gives, bit for bit: tests/test_gpu_local_parity.py), for fixed32
the word positions_in_kernel makes of it, itself checked against the exact image hp_reference.fixed_from_length.  Every
measured / bound ratio is recorded with record_measure (prefix local_parity_probe_)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import hp_reference as hp
import hp_sampler as hs
from hp_checks import (U64, Case, _acc_kind, _cell_dtype, _planted_positions, _ratio, _read, _weight_err,
                       density_bound, energy_bounds, gather_bound, solve_bounds)

pytestmark = pytest.mark.gpu


def _matrix():
    rng = np.random.default_rng(20261016)
    F64, F32, U = ("float64", "float"), ("float32", "float"), ("float32", "fixed32")
    rows = [
        # (format, shape, N, Ng, envs, accum, bpe)
        (F64, "CIC", 1, 4, 2, None, 0),
        (F32, "TSC", 7, 5, 2, None, 0),
        (U, "CIC", 100, 63, 2, None, 0),
        (F64, "TSC", 333, 64, 2, "float64", 2),
        (F32, "CIC", 1001, 65, 2, "packed", 3),
        (U, "TSC", 1023, 127, 2, "fix64", 0),
        (F64, "CIC", 2049, 128, 3, "fix64", 2),
        (F32, "TSC", 2047, 129, 2, "fix64", 0),
        (U, "CIC", 4095, 511, 2, "packed", 2),
        (F64, "TSC", 4096, 512, 2, None, 0),
        (F32, "CIC", 5000, 513, 2, None, 0),
        (F64, "CIC", 3000, 1023, 2, "float64", 0),
        (U, "TSC", 3001, 1024, 2, None, 0),
        (F32, "TSC", 3003, 1025, 2, None, 0),
        (F64, "CIC", 8192, 100, 2, None, 0),
        (F32, "TSC", 8193, 300, 2, None, 0),
        (F64, "CIC", 3000, 2722, 2, None, 0),
        (F32, "TSC", 3001, 3267, 2, None, 0),
        (U, "CIC", 3002, 3267, 2, None, 0),
        (F64, "TSC", 70000, 64, 1, None, 64),       # one environment, 35 workgroups: S = 4 accumulator sub-rows
        (F32, "CIC", 40001, 256, 2, None, 32),      # two environments, 20 workgroups each: S = 2
        (U, "TSC", 1 << 20, 64, 1, "fix64", 0),
    ]
    cases = []
    for (dtype, pos), shape, N, Ng, envs, accum, bpe in rows:
        L = float(rng.choice([1.0, 10.0, 50.0, 77.7]))
        if Ng in (100, 300):
            L = 50.0                       # singular in the reference's Sherman-Morrison solve
        cases.append(Case(dtype, pos, shape, N, Ng, L, envs, accum, bpe, ext=bool(rng.integers(0, 2))))
    return cases


CASES = _matrix()


def _make(oc, c):
    return oc.BatchedPIC(c.envs, c.N, c.Ng, n0=c.n0, L=c.L, dt=0.05, interpol=c.shape, dtype=c.dtype, accum_dtype=c.accum,
                         blocks_per_env=c.bpe, position_dtype=c.pos)


def _probe_positions(c, rng):
    """[envs, N] in the particle dtype, different in every environment: planted edges, far values (+-10^3 L), uniform."""
    X = rng.uniform(0, c.L, (c.envs, c.N))
    for e in range(c.envs):
        far = 1e3 * c.L + rng.uniform(0, c.L, 8)
        pts = np.concatenate([_planted_positions(c, rng).astype(np.float64), far, -far, [1e3 * c.L, -1e3 * c.L]])
        rng.shuffle(pts)
        m = min(pts.size, c.N)
        X[e, :m] = pts[:m]
    return X.astype(c.dtype)


def _held(c, X):
    """What the device holds for probe positions X: the dtype's wrap (float formats), positions_in_kernel's word (fixed32)."""
    if c.fixed:
        with np.errstate(invalid="ignore"):
            return hs._fixed_from_length(X.astype(np.float64), c.L)
    W = np.dtype(c.dtype).type
    with np.errstate(invalid="ignore"):
        xw = np.mod(np.mod(X, W(c.L)), W(c.L))
    return np.where(np.isfinite(xw), xw, W(0)).astype(c.dtype)


def _check_fixed_words(oc, c, X):
    """positions_in_kernel (through pic_set_particles, the probes' upload) against its float64 restatement bit for bit, and the
    restatement within one unit (on the circle) of the exact image: xs - floor(xs / L) L is off by at most
    |floor(xs/L)| L u64 <= 10^3 L 2^-53 = 2^-43 units of L 2^-32 plus the rounding of r / L (u64), then rint adds half a unit."""
    ld = _make(oc, c)
    try:
        ld._h.set_particles(X, np.zeros_like(X))
        got = ld.torch_views()["x_fixed"].cpu().numpy().view(np.uint32)
        assert ld.bad_count() == 0
    finally:
        ld.close()
    want = _held(c, X)
    assert np.array_equal(got, want), c
    exact = hp.fixed_from_length(X.astype(np.float64), c.L)
    d = (got.astype(np.int64) - exact.astype(np.int64)) % (1 << 32)
    d = np.minimum(d, (1 << 32) - d)
    assert np.all(d <= 1), (c, int(np.max(d)))
    _ratio("probe_fixed32_units", np.max(d), 1.0)


def _mesh_checks(c, e, n_dev, E_dev, ext, Xh, tag, phi_dev=None, pe_dev=None):
    n_hp, count = hp.deposit(Xh, c.Ng, c.L, c.n0, c.N, c.shape, _cell_dtype(c))
    bn = density_bound(c, n_hp, count)
    dn = np.abs(n_dev - n_hp).astype(float)
    r = float(np.max(dn / np.maximum(bn, 1e-300)))
    assert r <= 1.0, (tag, "n", r)
    _ratio("probe_n", r, 1.0)
    E_hp, phi_hp = hp.solve(n_dev, c.n0, c.L)
    Ef = E_hp if ext is None else E_hp + hp.as_ld(ext)
    bE, bphi, _ = solve_bounds(c, n_dev, E_dev)
    bE += U64 * float(np.max(np.abs(E_dev)))              # the addition of E_ext
    eE = float(np.max(np.abs(E_dev - Ef)))
    assert eE <= bE, (tag, "E_mesh", eE, bE)
    _ratio("probe_E_mesh", eE, bE)
    if phi_dev is not None:
        phi = phi_dev - np.mean(phi_dev.astype(hp.LD))
        ephi = float(np.max(np.abs(phi - phi_hp)))
        bphi += U64 * float(np.max(np.abs(phi_hp)))
        assert ephi <= bphi, (tag, "phi", ephi, bphi)
        _ratio("probe_phi", ephi, bphi)
    if pe_dev is not None:
        _, _, per = hp.energies(np.zeros(1), E_dev, c.L, c.N)
        _, bper, _ = energy_bounds(c, 0.0, per)
        err = abs(float(hp.LD(pe_dev) - per))
        assert err <= bper + 1e-300, (tag, "PE_reward", err, bper)
        _ratio("probe_PE_reward", err, bper)


def _shape_checks(c, idx, w, Xh, tag):
    jf, d = hp._cells(Xh, c.Ng, c.L, _cell_dtype(c))
    j = np.where(jf >= c.Ng, 0, jf)                       # the fold of j == Ng (csrc/pic_device.h: locate_in_box)
    offs, wx = hp.shape_weights(d, c.shape)
    if c.shape == "CIC":
        want = np.stack([j, np.where(j + 1 == c.Ng, 0, j + 1), np.zeros_like(j)])
    else:
        want = np.stack([np.where(j == 0, c.Ng - 1, j - 1), j, np.where(j + 1 == c.Ng, 0, j + 1)])
    assert np.array_equal(idx, want), (tag, "idx", int(np.sum(idx != want)))
    we = _weight_err(c)
    err = np.abs(w[: len(offs)] - wx).astype(float)
    assert np.all(err <= we), (tag, "w", float(np.max(err)) / we)
    _ratio("probe_w", np.max(err), we)
    if c.shape == "CIC":
        assert np.all(w[2] == 0), tag


def _gather_checks(c, got, mesh, Xh, tag, name):
    want = hp.gather(mesh, Xh, c.L, c.shape, _cell_dtype(c))
    b = gather_bound(c, mesh)
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) if got.size else 0.0
    assert err <= b + 1e-300, (tag, name, err, b)
    _ratio("probe_gather_" + name, err, b)


def _snapshot(env, c):
    views = env.torch_views()
    st = [_read(env, c, e, views) for e in range(c.envs)]
    return st, env.bad_count()


def _same(sa, sb, tag):
    for e, (a, b) in enumerate(zip(sa, sb)):
        for k in ("x", "v", "n", "E_mesh", "phi"):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (tag, e, k)
        for k in ("KE", "PE", "PE_reward"):
            assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (tag, e, k)


def _eval_field_device(env, c, X, E_ext):
    """pic_eval_field with PIC_DEVICE positions (torch device memory), through ctypes."""
    import torch
    h = env._h
    xt = torch.as_tensor(np.ascontiguousarray(X), device="cuda")
    n = np.empty((c.envs, c.Ng))
    E = np.empty_like(n)
    pe = np.empty(c.envs)
    e = None if E_ext is None else np.ascontiguousarray(E_ext)
    ptr = lambda a: None if a is None else C.c_void_p(a.__array_interface__["data"][0])   # noqa: E731
    torch.cuda.synchronize()
    h._chk(h.lib.pic_eval_field(h._h, C.c_void_p(xt.data_ptr()), 1, ptr(e), ptr(n), ptr(E), ptr(pe)))
    return n, E, pe


@pytest.mark.parametrize("case", CASES, ids=[f"p{i}" for i in range(len(CASES))])
def test_probes_against_longdouble(case):
    import ocplasma_amd as oc
    c = case
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    tag = repr(c)
    X = _probe_positions(c, rng)
    if c.fixed:
        _check_fixed_words(oc, c, X)
    Xh = _held(c, X)
    E_ext = rng.uniform(-0.5, 0.5, (c.envs, c.Ng)) if c.ext else None
    a, b = _make(oc, c), _make(oc, c)
    try:
        x0 = rng.uniform(0, c.L, (c.envs, c.N)).astype(c.dtype)
        v0 = rng.normal(0, 1, (c.envs, c.N)).astype(c.dtype)
        a.reset(x0, v0)
        b.reset(x0, v0)
        before, bad0 = _snapshot(a, c)
        assert bad0 == 0

        # 1. eval_field (the pinned-staging branch for small float states), 5. the other paths, bit for bit
        n1, E1, pe1 = a._h.eval_field(X, E_ext)
        nd, Ed, ped = _eval_field_device(a, c, X, E_ext)
        out = a._h.compute_E(X, E_ext, particles=True, shape=True)
        for e in range(c.envs):
            t = f"{tag} env {e}"
            _mesh_checks(c, e, n1[e], E1[e], None if E_ext is None else E_ext[e], Xh[e], t + " eval_field", pe_dev=pe1[e])
            _mesh_checks(c, e, out["n"][e], out["E_mesh"][e], None if E_ext is None else E_ext[e], Xh[e], t + " compute_E",
                         phi_dev=out["phi_mesh"][e])
            # 2. at the particles: E and phi gathered from the device's own meshes, indices exact, weights within bound
            _gather_checks(c, out["E"][e], out["E_mesh"][e], Xh[e], t, "E")
            _gather_checks(c, out["phi"][e], out["phi_mesh"][e], Xh[e], t, "phi")
            _shape_checks(c, out["idx"][e], out["w"][e], Xh[e], t)
        if _acc_kind(c) != "float64":        # float64 running sums are order-dependent in the last bits by design
            for name, got in (("device n", nd), ("device E", Ed), ("device pe", ped), ("compute_E n", out["n"]),
                              ("compute_E E_mesh", out["E_mesh"])):
                want = {"device n": n1, "device E": E1, "device pe": pe1, "compute_E n": n1, "compute_E E_mesh": E1}[name]
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (tag, name)

        # 3. gather_E at the handle's own particles, cic(env) of every environment
        st = [_read(a, c, e, a.torch_views()) for e in range(c.envs)]
        gE = a.gather_E()
        for e in range(c.envs):
            _gather_checks(c, gE[e], st[e]["E_mesh"], st[e]["x"], f"{tag} env {e}", "E_state")
            jl, jr, wl, wr = a._h.cic(e)
            cc = Case(c.dtype, c.pos, "CIC", c.N, c.Ng, c.L, c.envs, c.accum, c.bpe)
            _shape_checks(cc, np.stack([jl, jr, np.zeros_like(jl)]), np.stack([wl, wr, np.zeros_like(wl)]), st[e]["x"],
                          f"{tag} env {e} cic")
            if c.shape == "CIC" and not c.fixed:
                o2 = a._h.compute_E(np.stack([s["x"] for s in st]), None, particles=False, shape=True)
                assert np.array_equal(o2["idx"][e][:2], np.stack([jl, jr])), (tag, e, "cic idx")
                assert np.array_equal(o2["w"][e][:2].view(np.uint8), np.stack([wl, wr]).view(np.uint8)), (tag, e, "cic w")

        # non-finite probe positions, in a call of their own: deposited at x = 0, counted nowhere
        Xn = X.copy()
        Xn[:, : min(3, c.N)] = np.array([np.nan, np.inf, -np.inf], dtype=c.dtype)[: min(3, c.N)]
        nn, En, _ = a._h.eval_field(Xn, None)
        Xnh = _held(c, Xn)
        for e in range(c.envs):
            _mesh_checks(c, e, nn[e], En[e], None, Xnh[e], f"{tag} env {e} non-finite")
        on = a._h.compute_E(Xn, None, particles=False, shape=True)
        for e in range(c.envs):
            _shape_checks(c, on["idx"][e], on["w"][e], Xnh[e], f"{tag} env {e} non-finite")

        # 7. nothing changed: state, fields, energies, bad_count; the next step bit-identical to the twin's
        after, bad1 = _snapshot(a, c)
        _same(before, after, tag + " after probes")
        assert bad1 == 0, (tag, "bad_count after probes", bad1)
        # (not for the float64 accumulator: two handles' running sums may differ in the last bits by design)
        twin = _acc_kind(c) != "float64"
        a.step(None, 1)
        b.step(None, 1)
        if twin:
            _same(_snapshot(b, c)[0], _snapshot(a, c)[0], tag + " step after probes")
        # a probe inside an open staged step
        a._h.step_stage(1)
        b._h.step_stage(1)
        a._h.eval_field(Xn, E_ext)
        a._h.compute_E(X, None, particles=True, shape=True)
        for h in (a, b):
            h._h.step_stage(2)
            h._h.step_stage(3)
        sa, bada = _snapshot(a, c)
        if twin:
            _same(_snapshot(b, c)[0], sa, tag + " staged step with probes")
        assert bada == 0 and b.bad_count() == 0, (tag, bada)
    finally:
        a.close()
        b.close()


SOLVE_NG = sorted({4, 5, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2722, 3267, 100, 300})


@pytest.mark.parametrize("Ng", SOLVE_NG)
def test_solve_poisson(Ng):
    """Zero-sum right-hand sides against hp.solve with solve_bounds (L = 50 at Ng = 100, 300: singular for the reference's
    Sherman-Morrison solve); then a right-hand side with a non-zero sum, which the header refuses to define: the device applies
    the scan formula to it as given (no projection, no error), i.e. hp.solve of the same rhs."""
    import ocplasma_amd as oc
    rng = np.random.default_rng(Ng)
    L = 50.0 if Ng in (100, 300) else float(rng.choice([1.0, 10.0, 77.7]))
    env = oc.BatchedPIC(2, 16, Ng, L=L, dt=0.05, dtype="float64" if Ng <= 2722 else "float32")   # (the LDS limit of the steps)
    c = Case("float64", "float", "CIC", 16, Ng, L, 2, n0=0.0)
    try:
        r = rng.normal(0, 1, (2, Ng))
        rhs = r - r.mean(axis=1, keepdims=True)
        phi, E = env._h.solve_poisson(rhs)
        for e in range(2):
            E_hp, phi_hp = hp.solve(rhs[e], 0.0, L)
            bE, bphi, _ = solve_bounds(c, rhs[e], E[e])
            eE = float(np.max(np.abs(E[e] - E_hp)))
            assert eE <= bE, (Ng, e, eE, bE)
            _ratio("probe_solve_E", eE, bE)
            ph = phi[e] - np.mean(phi[e].astype(hp.LD))
            ephi = float(np.max(np.abs(ph - phi_hp)))
            bphi += U64 * float(np.max(np.abs(phi_hp)))
            assert ephi <= bphi, (Ng, e, ephi, bphi)
            _ratio("probe_solve_phi", ephi, bphi)
        off = rhs + np.array([[0.25], [-1.0]])
        phi2, E2 = env._h.solve_poisson(off)
        for e in range(2):
            E_hp, _ = hp.solve(off[e], 0.0, L)
            bE, _, _ = solve_bounds(c, off[e], E2[e])
            assert float(np.max(np.abs(E2[e] - E_hp))) <= bE, (Ng, e, "non-zero sum")
    finally:
        env.close()


def test_state_gradient_with_wrapping():
    """PIC.compute_state_gradient on float64 states outside [0, L) against [v; -gather(solve(deposit(x)))] in longdouble:
    the deposit within density_bound, the field through the linear solve (|dE_mesh| <= 2 dx sum dn + solve rounding), at the
    particle sum|w| |dE_mesh| + gather_bound."""
    import ocplasma_amd as oc
    N, Ng, L = 3000, 128, 50.0
    rng = np.random.default_rng(4)
    np.random.seed(4)
    sim = oc.PIC(N=N, N_mesh=Ng, n0=1.0, L=L, dt=0.1, A=0.1, n_mode=2, interpol="CIC",
                 init_dist=oc.BumpOnTail(a=0.2, v0=3.0, sigma=1.0, n_samples=N, L=L))
    c = Case("float64", "float", "CIC", N, Ng, L)
    for ext in (None, rng.uniform(-0.3, 0.3, Ng)):
        x = rng.uniform(-3 * L, 4 * L, N)
        x[:4] = [-L, 2 * L, -1e-300, 1e3 * L + 0.5]
        v = rng.normal(0, 1, N)
        eta = np.concatenate([x, v]).reshape(-1, 1)
        out = sim.compute_state_gradient(eta.copy(), ext)
        assert np.array_equal(out[:N, 0], v)
        xw = np.mod(np.mod(x, L), L)
        n_hp, count = hp.deposit(xw, Ng, L, 1.0, N, "CIC", np.float64)
        E_hp, _ = hp.solve(n_hp, 1.0, L)
        if ext is not None:
            E_hp = E_hp + hp.as_ld(ext)
        want = -hp.gather(E_hp, xw, L, "CIC", np.float64)
        dx = L / Ng
        dn = density_bound(c, n_hp, count)
        bE, _, _ = solve_bounds(c, n_hp.astype(float), E_hp.astype(float))
        dE = 2 * dx * float(np.sum(dn)) + bE + 2 * U64 * float(np.max(np.abs(E_hp)))
        b = dE + gather_bound(c, E_hp.astype(float)) + U64 * float(np.max(np.abs(E_hp)))
        err = float(np.max(np.abs(out[N:, 0] - want)))
        assert err <= b, (err, b)
        _ratio("probe_state_gradient", err, b)


@pytest.mark.parametrize("dtype,pos", [("float64", "float"), ("float32", "float"), ("float32", "fixed32")])
def test_non_finite_probe_positions_leave_bad_count(dtype, pos):
    """pic_bad_count describes the state's particles (include/picstep.h): probes with NaN / +-inf positions -- through the
    pinned staging, the regular upload and compute_E -- must not add to it, and the state stays healthy."""
    import ocplasma_amd as oc
    N, Ng, L = 512, 64, 10.0
    rng = np.random.default_rng(9)
    env = oc.BatchedPIC(2, N, Ng, L=L, dt=0.05, dtype=dtype, position_dtype=pos)
    try:
        env.reset(rng.uniform(0, L, (2, N)), rng.normal(0, 1, (2, N)))
        assert env.bad_count() == 0
        X = rng.uniform(0, L, (2, N)).astype(dtype)
        X[:, :3] = np.array([np.nan, np.inf, -np.inf], dtype=dtype)
        env._h.eval_field(X)
        env._h.compute_E(X, None, particles=True, shape=True)
        assert env.bad_count() == 0, ("probe counted into the state's bad_count", env.bad_count())
        env.step(None, 1)
        assert env.bad_count() == 0
    finally:
        env.close()
