"""The fluid moments on the mesh without a GPU: the C declarations of pic_moments*, the invariants of the
restatement (tests/hp_moments.py), its hand gather against autograd, and the policy entry's argument check."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import hp_adjoint as ha
import hp_moments as hm
from conftest import rel_err
from oracle import pic_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = hm.LD


def test_moments_are_declared_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int pic_moments(pic_handle* h, int mem_kind, double* m);" in flat
    assert "int pic_moments_vjp(pic_handle* h, const double* cot_m, int mem_kind, void* g_x, void* g_v);" in flat
    assert ("int pic_tape_moments_cot(pic_handle* h, const double* cot_m, int mem_kind, int64_t first_step, "
            "int64_t nsteps);") in flat
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _abi.SIGNATURES["pic_moments"] == [vp, ci, vp]
    assert _abi.SIGNATURES["pic_moments_vjp"] == [vp, vp, ci, vp, vp]
    assert _abi.SIGNATURES["pic_tape_moments_cot"] == [vp, vp, ci, i64, i64]
    for name in ("moments", "moments_vjp", "tape_moments_cot"):
        assert callable(getattr(_abi.Handle, name)), name
    # nothing existing moved: pic_tape_info keeps its seven int64
    assert ctypes.sizeof(_abi.PicTapeInfo) == 56
    lib = ctypes.CDLL(_build.build_library())
    for name in ("pic_moments", "pic_moments_vjp", "pic_tape_moments_cot"):
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_python_entries_take_the_moments():
    import inspect
    from ocplasma_amd.env.batched import BatchedPIC, TapeWalk
    from ocplasma_amd.env.pic import PIC
    for name in ("moments", "moments_torch", "fluid", "moments_vjp"):
        assert callable(getattr(BatchedPIC, name)), name
    assert callable(PIC.fluid_moments)
    assert "d_moments" in inspect.signature(BatchedPIC.backward).parameters
    assert "d_moments" in inspect.signature(TapeWalk.step).parameters
    assert "d_moments0" in inspect.signature(TapeWalk.end).parameters


@pytest.mark.parametrize("shape", ["CIC", "TSC"])
@pytest.mark.parametrize("N,Ng", [(3001, 64), (5000, 250)])
def test_restatement_invariants(N, Ng, shape):
    L, n0 = 50.0, 1.0
    x, v = po.synthetic_bump_on_tail(N, L, seed=4)
    m = hm.moments_ld(x, v, Ng, L, n0, shape, cell_dtype=np.float64)
    dx = LD(L) / LD(Ng)
    s = LD(n0) * LD(L) / LD(N) / dx
    vl = np.asarray(v).astype(LD)
    # sum m0 = n0 Ng, sum m2 N dx / (2 n0 L) = KE, sum m1 / s = sum v: longdouble sums of N terms, eps 5.4e-20 each
    assert abs(m[0].sum() / (LD(n0) * Ng) - 1) < 1e-15
    assert abs(m[2].sum() * (LD(N) * dx / (2 * LD(n0) * LD(L))) / (LD(0.5) * (vl * vl).sum()) - 1) < 1e-15
    assert abs(m[1].sum() / s - vl.sum()) < 1e-15 * np.abs(vl).sum()
    if shape == "CIC":     # the float64 torch restatement is the same quantity
        S = ha.Setup(N, Ng, L, n0, 0.1)
        mt = hm.moments_torch(torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(v, dtype=np.float64)), S)
        for k in range(3):
            assert rel_err(mt[k].numpy(), m[k].astype(np.float64)) < 1e-12, k


@pytest.mark.parametrize("N,Ng", [(3001, 64), (2000, 250)])
def test_hand_vjp_matches_autograd(N, Ng):
    """Both are float64 evaluations of the same formula: 1e-12 in relative norm."""
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x, v = po.synthetic_bump_on_tail(N, S.L, seed=9)
    g = np.random.default_rng(2).standard_normal((3, Ng))
    ax, av = hm.autograd_vjp(x, v, g, S)
    hx, hv = hm.hand_vjp(x, v, g, S)
    assert np.linalg.norm(hx - ax) < 1e-12 * np.linalg.norm(ax)
    assert np.linalg.norm(hv - av) < 1e-12 * np.linalg.norm(av)


def test_vjp_matches_central_differences():
    N, Ng = 1500, 32
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x, v = (np.asarray(a, dtype=np.float64) for a in po.synthetic_bump_on_tail(N, S.L, seed=3))
    rng = np.random.default_rng(5)
    g = rng.standard_normal((3, Ng))
    gx, gv = hm.hand_vjp(x, v, g, S)
    J = lambda xx, vv: float((hm.moments_torch(torch.as_tensor(xx), torch.as_tensor(vv), S).numpy() * g).sum())  # noqa: E731
    eps = 1e-7                                   # (the CIC moments are continuous: a particle that crosses a cell edge costs O(eps))
    dxx, dvv = rng.standard_normal(N), rng.standard_normal(N)
    fd = (J(x + eps * dxx, v + eps * dvv) - J(x - eps * dxx, v - eps * dvv)) / (2 * eps)
    an = float((gx * dxx).sum() + (gv * dvv).sum())
    assert abs(fd - an) <= 1e-5 * abs(an), (fd, an)


def test_rollout_policy_still_refuses_an_unknown_observation():
    from ocplasma_amd.env import grad
    env = types.SimpleNamespace(max_mode=2, N_mesh=64, num_envs=1, device=0)
    with pytest.raises(ValueError, match="observe"):
        grad.rollout_policy(env, lambda o: o, 3, observe="nonsense")
