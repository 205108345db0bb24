"""Forward mode of the fluid moments without a GPU: the restatement (tests/hp_moments_jvp.py) against torch
forward-mode AD and against the reverse mode's gather, its invariants, the C declarations, the bindings and the build."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import hp_adjoint as ha
import hp_moments as hm
import hp_moments_jvp as hj
from oracle import pic_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 3


def _rel(a, b):
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def _state(N, S, seed):
    x, v = (np.asarray(a, dtype=np.float64) for a in po.synthetic_bump_on_tail(N, S.L, seed=seed))
    rng = np.random.default_rng(seed + 100)
    return x, v, rng.standard_normal(N), rng.standard_normal(N)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Ng", [(3001, 64), (2000, 250)])
def test_hand_jvp_matches_forward_ad(N, Ng):
    """Both are float64 evaluations of the same formula."""
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x, v, dx, dv = _state(N, S, 3)
    for a, b in ((dx, dv), (dx, None), (None, dv)):
        assert _rel(hj.hand_jvp(x, v, a, b, S), hj.torch_jvp(x, v, a, b, S)) < 1e-10
    # and of the longdouble evaluation on the same cells
    assert _rel(hj.hand_jvp(x, v, dx, dv, S), hj.jvp_ld(x, v, dx, dv, Ng, S.L).astype(np.float64)) < 1e-10


@pytest.mark.parametrize("N,Ng", [(3001, 64), (2000, 250)])
def test_hand_jvp_is_dual_to_the_hand_vjp(N, Ng):
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x, v, dx, dv = _state(N, S, 5)
    c = np.random.default_rng(7).standard_normal((3, Ng))
    gx, gv = hm.hand_vjp(x, v, c, S)
    lhs = float((c * hj.hand_jvp(x, v, dx, dv, S)).sum())
    rhs = float((gx * dx).sum() + (gv * dv).sum())
    assert abs(lhs - rhs) < 1e-12 * max(abs(lhs), abs(rhs))


@pytest.mark.parametrize("N,Ng", [(3001, 64), (2000, 250)])
def test_invariants_of_the_restatement(N, Ng):
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x, v, dx, dv = _state(N, S, 9)
    m = hj.jvp_ld(x, v, dx, dv, Ng, S.L)
    LD = hj.LD
    scale = LD(1.0) * LD(S.L) / LD(N) / (LD(S.L) / LD(Ng))
    # sum_j dm0_j = 0: every particle adds -iota and +iota
    assert abs(m[0].sum()) < 1e-15 * np.abs(m[0]).sum()
    # sum_j dm2_j N dx / (2 n0 L) = sum_i v_i dv_i (the weights sum to one, the iota terms cancel)
    want = (v.astype(LD) * dv.astype(LD)).sum()
    assert abs(m[2].sum() / (2 * scale) - want) < 1e-15 * np.abs(v * dv).sum()


def test_rollout_restatement_matches_forward_ad():
    N, Ng, T = 1500, 32, 3
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x, v, dx, dv = _state(N, S, 11)
    rng = np.random.default_rng(13)
    ext, de = 0.3 * rng.standard_normal((T, Ng)), rng.standard_normal((T, Ng))
    got = hj.rollout_hand_jvp(x, v, ext, S, d_ext=de, d_x0=dx, d_v0=dv)
    want = hj.rollout_torch_jvp(x, v, ext, S, d_ext=de, d_x0=dx, d_v0=dv)
    assert got.shape == (T, 3, Ng)
    assert _rel(got, want) < 1e-10


# ---- declarations, bindings, build -------------------------------------------------------------------------------------------------
DECLS = (
    "int pic_moments_jvp(pic_handle* h, int K, const void* d_x, const void* d_v, int mem_kind, double* d_m);",
    "int pic_tape_moments_start(pic_handle* h);",
    "int pic_tape_moments(pic_handle* h, int mem_kind, double* m);",
    "int pic_tape_tangent_moments(pic_handle* h, int K, const double* d_ext, const double* d_actions, const void* d_x0, "
    "const void* d_v0, int mem_kind, double* d_hist, void* d_x, void* d_v, double* d_E_mesh, double* d_kl, double* d_moments);",
)
NAMES = {"pic_moments_jvp": 6, "pic_tape_moments_start": 1, "pic_tape_moments": 3, "pic_tape_tangent_moments": 13}


def test_entries_are_declared_bound_and_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for d in DECLS:
        assert d in flat, d
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    assert ctypes.sizeof(_abi.PicTapeInfo) == 56
    for name, n in NAMES.items():
        assert len(_abi.SIGNATURES[name]) == n, name       # (the arguments of the C prototypes above, the handle included)
    assert len(_abi.SIGNATURES["pic_tape_tangent"]) == 11 and len(_abi.SIGNATURES["pic_tape_tangent_kl"]) == 12
    for name in ("moments_jvp", "tape_moments_start", "tape_moments", "tape_tangent_moments"):
        assert callable(getattr(_abi.Handle, name)), name
    lib = ctypes.CDLL(_build.build_library())
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_new_kernels_are_scratch_free():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    mine = {k: r for k, r in res.items() if "moments_jvp_" in k}
    kinds = {k2 for k2 in ("moments_jvp_max_kernel", "moments_jvp_deposit_kernel", "moments_jvp_finish_kernel")
             if any(k2 in k for k in mine)}
    assert len(kinds) == 3, sorted(mine)
    assert len(mine) == 7, sorted(mine)                     # max and deposit for up to 1, 4 and 8 directions, one finish
    for k, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (k, r)


def test_python_keywords_exist_and_default_to_off():
    from ocplasma_amd.env import grad
    from ocplasma_amd.env.batched import BatchedPIC
    assert callable(BatchedPIC.moments_jvp) and callable(BatchedPIC.tape_moments)
    p = inspect.signature(BatchedPIC.moments_jvp).parameters
    assert p["d_x"].default is None and p["d_v"].default is None
    for fn in (BatchedPIC.start_tape, BatchedPIC.taping, BatchedPIC.tangent, grad.rollout, grad.rollout_ext):
        assert inspect.signature(fn).parameters["moments"].default is False, fn
    assert inspect.signature(BatchedPIC.tape_moments).parameters["on_device"].default is False
