"""The per-step smoothed KL of a taped rollout without a GPU: the hand reverse equations with the KL's gather
injected behind every step (tests/hp_tape_kl.py) against autograd of the restatement, autograd against central differences, and
the C declarations of pic_tape_kl_*."""
import ctypes
import os
import re

import numpy as np
import pytest

import hp_adjoint as ha
import hp_phase as hp
import hp_tape_kl as hk
from conftest import rel_err
from oracle import pic_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(N, Ng, T, nx, nv, vmin, vmax, seed):
    rng = np.random.default_rng(seed)
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    G = hp.Grid(nx, nv, S.L, vmin, vmax, N, S.n0)
    x0, v0 = po.synthetic_bump_on_tail(N, S.L, seed=seed)
    ext = 0.05 * rng.standard_normal((T, Ng))
    feq = rng.uniform(0.0, 2.0 / (S.L * (vmax - vmin)), (nx, nv))
    cot_kl, cot = rng.standard_normal(T), rng.standard_normal((T, 3))
    cx, cv = rng.standard_normal(N), rng.standard_normal(N)
    return S, G, np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64), ext, feq, cot_kl, cot, cx, cv, rng


# (the second grid's velocity range is narrower than the particles': dropped particles and clamped half-bins occur)
@pytest.mark.parametrize("N,Ng,T,nx,nv,vmin,vmax", [(2000, 64, 3, 16, 12, -6.0, 6.0), (3000, 250, 5, 7, 33, -2.0, 3.0)])
def test_hand_adjoint_with_the_kl_injected_matches_autograd(N, Ng, T, nx, nv, vmin, vmax):
    S, G, x0, v0, ext, feq, cot_kl, cot, cx, cv, _ = _problem(N, Ng, T, nx, nv, vmin, vmax, 5)
    if vmax < 6.0:
        assert np.any(v0 > vmax) and np.any(v0 < vmin)
    # every cotangent at once
    ge, gx, gv = hk.autograd_vjp(x0, v0, ext, S, G, feq, cot_kl, cot, cx, cv)
    he, hx, hv = hk.hand_vjp(x0, v0, ext, S, G, feq, cot_kl, cot, cx, cv)
    assert rel_err(he, ge) < 1e-10 and rel_err(hx, gx) < 1e-10 and rel_err(hv, gv) < 1e-10
    # the KL alone
    ge, gx, gv = hk.autograd_vjp(x0, v0, ext, S, G, feq, cot_kl)
    he, hx, hv = hk.hand_vjp(x0, v0, ext, S, G, feq, cot_kl)
    assert rel_err(he, ge) < 1e-10 and rel_err(hx, gx) < 1e-10 and rel_err(hv, gv) < 1e-10
    # no KL cotangent: hp_adjoint's own reverse pass
    he, hx, hv = hk.hand_vjp(x0, v0, ext, S, G, feq, np.zeros(T), cot, cx, cv)
    pe, px, pv = ha.hand_vjp(x0, v0, ext, S, cot, cx, cv)
    assert np.array_equal(he, pe) and np.array_equal(hx, px) and np.array_equal(hv, pv)


def test_kl_trace_is_the_kl_of_every_post_step_state():
    import torch
    S, G, x0, v0, ext, feq, *_ = _problem(1500, 64, 4, 16, 16, -6.0, 6.0, 3)
    trace = hk.kl_trace(x0, v0, ext, S, G, feq)
    x, v = torch.as_tensor(x0), torch.as_tensor(v0)
    with torch.no_grad():
        for t in range(4):
            x, v, *_ = ha.step(x, v, torch.as_tensor(ext[t]), S)
            assert trace[t] == float(hp.kl(hp.density(x[None], v[None], G), torch.as_tensor(feq), G)[0])


@pytest.mark.parametrize("N,Ng,T", [(2000, 64, 3), (1000, 32, 5)])
def test_vjp_matches_central_differences_of_the_running_kl(N, Ng, T):
    """A directional central difference of sum_t k-bar_t KL~_t (the unquantised density: no rounding noise) against the
    vector-Jacobian product; the step size and bound of test_adjoint_cpu.py's check."""
    S, G, x0, v0, ext, feq, cot_kl, _, _, _, rng = _problem(N, Ng, T, 16, 12, -6.0, 6.0, 11)
    ge, gx, gv = hk.autograd_vjp(x0, v0, ext, S, G, feq, cot_kl)
    eps = 1e-6
    for _ in range(3):
        de, dxx, dvv = rng.standard_normal(ext.shape), rng.standard_normal(N), rng.standard_normal(N)
        Jp = hk.objective(x0 + eps * dxx, v0 + eps * dvv, ext + eps * de, S, G, feq, cot_kl)
        Jm = hk.objective(x0 - eps * dxx, v0 - eps * dvv, ext - eps * de, S, G, feq, cot_kl)
        fd = (Jp - Jm) / (2 * eps)
        an = float((ge * de).sum() + (gx * dxx).sum() + (gv * dvv).sum())
        assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-12), (fd, an)


def test_tape_kl_is_declared_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int pic_tape_kl_start(pic_handle* h, const pic_phase_spec* spec);" in flat
    assert "int pic_tape_kl(pic_handle* h, int mem_kind, double* kl);" in flat
    assert ("int pic_tape_kl_cot(pic_handle* h, const double* cot_kl, int mem_kind, int64_t first_step, "
            "int64_t nsteps);") in flat
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _abi.SIGNATURES["pic_tape_kl_start"] == [vp, ctypes.POINTER(_abi.PicPhaseSpec)]
    assert _abi.SIGNATURES["pic_tape_kl"] == [vp, ci, vp]
    assert _abi.SIGNATURES["pic_tape_kl_cot"] == [vp, vp, ci, i64, i64]
    # nothing existing moved: pic_tape_info keeps its seven int64
    assert ctypes.sizeof(_abi.PicTapeInfo) == 56
    lib = ctypes.CDLL(_build.build_library())
    for name in ("pic_tape_kl_start", "pic_tape_kl", "pic_tape_kl_cot"):
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_python_entries_take_the_kl():
    import inspect
    from ocplasma_amd.env import grad
    from ocplasma_amd.env.batched import BatchedPIC, TapeWalk
    assert "kl" in inspect.signature(BatchedPIC.start_tape).parameters
    assert "d_KL" in inspect.signature(BatchedPIC.backward).parameters
    assert "d_kl" in inspect.signature(TapeWalk.step).parameters
    assert callable(BatchedPIC.tape_kl)
    for name in ("rollout", "rollout_ext", "rollout_feedback", "rollout_policy"):
        p = inspect.signature(getattr(grad, name)).parameters
        assert "kl" in p and p["kl"].default is None, name
