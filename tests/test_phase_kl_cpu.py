"""The smoothed phase-space KL without a GPU: the restatement's hand vector-Jacobian product against autograd and
central differences, its mass against the in-range count, and the C declarations of pic_phase_kl_smooth*."""
import ctypes
import os
import re

import torch

import hp_phase as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sample(E, N, L, vmin, vmax, seed, spill=0.05):
    """Particles on [0, L) x a Gaussian-ish v that spills a little beyond [vmin, vmax] (dropped) and into the clamped half-bins."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(E, N, generator=g, dtype=torch.float64) * L
    span = vmax - vmin
    v = vmin - spill * span + torch.rand(E, N, generator=g, dtype=torch.float64) * (1 + 2 * spill) * span
    return x, v


def _target(G, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(G.nx, G.nv, generator=g, dtype=torch.float64) * (2.0 / (G.L * (G.vmax - G.vmin)))


def test_hand_vjp_equals_autograd():
    for nx, nv, E, per_env in ((16, 12, 2, False), (7, 33, 3, True), (1, 5, 1, False)):
        G = hp.Grid(nx, nv, 50.0, -6.0, 6.0, 3000)
        x, v = _sample(E, G.N, G.L, G.vmin, G.vmax, seed=nx + nv)
        feq = torch.stack([_target(G, e) for e in range(E)]) if per_env else _target(G, 7)
        d = torch.linspace(0.5, 1.5, E, dtype=torch.float64)
        hx, hv = hp.vjp(x, v, feq, d, G)
        ax, av = hp.autograd_vjp(x, v, feq, d, G)
        scale = max(float(ax.abs().max()), float(av.abs().max()))
        assert float((hx - ax).abs().max()) <= 1e-12 * scale
        assert float((hv - av).abs().max()) <= 1e-12 * scale
        assert float(hv[(v < G.vmin + G.dv / 2) | (v > G.vmax - G.dv / 2)].abs().max()) == 0.0   # clamped and dropped: no slope


def test_vjp_agrees_with_central_differences_away_from_bin_edges():
    G = hp.Grid(12, 10, 50.0, -5.0, 5.0, 400)
    x, v = _sample(1, G.N, G.L, G.vmin, G.vmax, seed=3, spill=0.0)
    feq = _target(G, 1)
    d = torch.ones(1, dtype=torch.float64)
    gx, gv = hp.vjp(x, v, feq, d, G)
    h = 1e-6
    _, _, _, _, _, fx, fv, slope = hp.locate(x, v, G)
    ok = (fx > 1e-3) & (fx < 1 - 1e-3) & (((fv > 1e-3) & (fv < 1 - 1e-3)) | ~slope)
    # the derivative is that of the unquantised weights: differences of the unquantised density (no rounding noise)
    J = lambda xx, vv: float(hp.kl(hp.density_smooth(xx, vv, G), feq, G)[0])  # noqa: E731
    idx = torch.nonzero(ok[0]).ravel()[:20]
    assert len(idx) == 20
    for k in idx.tolist():
        for arr, g in ((x, gx), (v, gv)):
            p, m = arr.clone(), arr.clone()
            p[0, k] += h
            m[0, k] -= h
            fd = (J(p, v) - J(m, v)) / (2 * h) if arr is x else (J(x, p) - J(x, m)) / (2 * h)
            assert abs(float(g[0, k]) - fd) < 1e-7, (k, float(g[0, k]), fd)


def test_mass_equals_the_in_range_count():
    G = hp.Grid(250, 250, 50.0, -4.0, 4.0, 5000)
    x, v = _sample(3, G.N, G.L, G.vmin, G.vmax, seed=11, spill=0.1)
    c = hp.counts(x, v, G)
    inside = ((x >= 0) & (x <= G.L) & (v >= G.vmin) & (v <= G.vmax)).sum(dim=1)
    assert torch.equal(c.sum(dim=(1, 2)), inside * (1 << (G.abits + G.bbits)))   # integer mass, exactly
    f = hp.density(x, v, G)
    mass = f.sum(dim=(1, 2)) * G.dx * G.dv
    assert float((mass - G.n0 * inside.to(torch.float64) / G.N).abs().max()) < 1e-13


def test_particles_at_bin_centres_give_the_histogram():
    """Power-of-two bin widths and particles at bin centres: f~ is estimate_f's histogram, bit for bit."""
    G = hp.Grid(32, 32, 64.0, -16.0, 16.0, 2048)
    g = torch.Generator().manual_seed(5)
    i = torch.randint(0, 32, (1, G.N), generator=g)
    j = torch.randint(0, 32, (1, G.N), generator=g)
    x = (i.to(torch.float64) + 0.5) * G.dx
    v = G.vmin + (j.to(torch.float64) + 0.5) * G.dv
    hist = torch.zeros(32 * 32, dtype=torch.float64).index_add_(0, (i * 32 + j).ravel(), torch.ones(G.N, dtype=torch.float64))
    assert torch.equal(hp.density(x, v, G)[0], hist.reshape(32, 32) * G.norm)


def test_phase_kl_smooth_is_declared_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int pic_phase_kl_smooth(pic_handle* h, const pic_phase_spec* spec, int mem_kind, double* kl, double* f);" in flat
    assert ("int pic_phase_kl_smooth_vjp(pic_handle* h, const pic_phase_spec* spec, const double* cot_kl, int mem_kind, "
            "void* g_x, void* g_v);") in flat
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    vp, ci = ctypes.c_void_p, ctypes.c_int
    sp = ctypes.POINTER(_abi.PicPhaseSpec)
    assert _abi.SIGNATURES["pic_phase_kl_smooth"] == [vp, sp, ci, vp, vp]
    assert _abi.SIGNATURES["pic_phase_kl_smooth_vjp"] == [vp, sp, vp, ci, vp, vp]
    body = hdr[hdr.index("typedef struct pic_phase_spec {"):hdr.index("} pic_phase_spec;")]
    fields = [f for decl in re.findall(r"^\s*(?:int32_t|double|const double\*)\s+([\w, ]+);", body, re.M)
              for f in decl.replace(" ", "").split(",")]
    assert fields == [f[0] for f in _abi.PicPhaseSpec._fields_], fields
    assert ctypes.sizeof(_abi.PicPhaseSpec) == 40
    lib = ctypes.CDLL(_build.build_library())
    for name in ("pic_phase_kl_smooth", "pic_phase_kl_smooth_vjp"):
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_batched_pic_has_the_smooth_kl_methods():
    from ocplasma_amd.env.batched import BatchedPIC
    for name in ("phase_density_smooth", "kl_smooth", "kl_smooth_grad"):
        assert callable(getattr(BatchedPIC, name)), name
