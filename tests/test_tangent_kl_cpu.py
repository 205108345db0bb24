"""The forward mode of the per-step smoothed KL without a GPU: the hand tangent equations with the KL's dot product
behind every step (tests/hp_tangent_kl.py) against torch forward-mode AD of the restatement, their duality with the hand reverse
pass of tests/hp_tape_kl.py, and the C declarations of pic_phase_kl_smooth_jvp and pic_tape_tangent_kl."""
import ctypes
import os
import re

import numpy as np
import pytest

import hp_adjoint as ha
import hp_phase as hp
import hp_tangent_kl as htk
import hp_tape_kl as hk
from conftest import ROOT, rel_err
from oracle import pic_oracle as po

NG, T = 32, 3
# the bump-on-tail velocities reach past [-1.5, 3]: particles are dropped there, and some fall in the clamped half-bins
CASES = [(301, 16, 16, -1.5, 3.0), (1000, 16, 16, -1.5, 3.0), (301, 8, 24, -1.5, 3.0), (1000, 8, 24, -1.5, 3.0)]


def _problem(N, nx, nv, vmin, vmax, seed):
    rng = np.random.default_rng(seed)
    S = ha.Setup(N, NG, 50.0, 1.0, 0.1)
    G = hp.Grid(nx, nv, S.L, vmin, vmax, N, S.n0)
    x0, v0 = (np.asarray(a, dtype=np.float64) for a in po.synthetic_bump_on_tail(N, S.L, seed=seed))
    ext = 0.05 * rng.standard_normal((T, NG))
    feq = rng.uniform(0.0, 2.0 / (S.L * (vmax - vmin)), (nx, nv))
    if vmax < 6.0:
        half = 0.5 * G.dv
        assert np.any(v0 > vmax) and np.any(v0 < vmin), "no particle is dropped"
        assert np.any((v0 >= vmin) & (v0 < vmin + half)) and np.any((v0 <= vmax) & (v0 > vmax - half)), "no clamped half-bin"
    return S, G, x0, v0, ext, feq, rng


@pytest.mark.parametrize("N,nx,nv,vmin,vmax", CASES)
@pytest.mark.parametrize("which", ["x0", "v0", "ext", "all"])
def test_hand_tangent_with_the_kl_matches_torch_forward_mode(N, nx, nv, vmin, vmax, which):
    S, G, x0, v0, ext, feq, rng = _problem(N, nx, nv, vmin, vmax, 3)
    u = {"d_x0": rng.standard_normal(N), "d_v0": rng.standard_normal(N), "d_ext": 0.1 * rng.standard_normal((T, NG))}
    if which != "all":
        u = {k: a for k, a in u.items() if k == "d_" + which}
    hh, hkl, hx, hv = htk.hand_jvp(x0, v0, ext, S, G, feq, **u)
    th, tkl, tx, tv = htk.torch_jvp(x0, v0, ext, S, G, feq, **u)
    assert np.any(tkl != 0.0)
    assert rel_err(hkl, tkl) < 1e-10, rel_err(hkl, tkl)
    assert rel_err(hh, th) < 1e-10 and rel_err(hx, tx) < 1e-10 and rel_err(hv, tv) < 1e-10


@pytest.mark.parametrize("N,nx,nv,vmin,vmax", CASES)
def test_hand_tangent_with_the_kl_is_dual_to_the_hand_adjoint(N, nx, nv, vmin, vmax):
    """<k-bar, dKL> + <a-bar, dhist> = <e-bar, de> + <x-bar_0, dx_0> + <v-bar_0, dv_0>."""
    S, G, x0, v0, ext, feq, rng = _problem(N, nx, nv, vmin, vmax, 8)
    de, dx, dv = 0.1 * rng.standard_normal((T, NG)), rng.standard_normal(N), rng.standard_normal(N)
    cot_kl, cot = rng.standard_normal(T), rng.standard_normal((T, 3))
    hh, hkl, _, _ = htk.hand_jvp(x0, v0, ext, S, G, feq, de, dx, dv)
    ge, gx, gv = hk.hand_vjp(x0, v0, ext, S, G, feq, cot_kl, cot)
    lhs = float((hkl * cot_kl).sum() + (hh * cot).sum())
    rhs = float((de * ge).sum() + (dx * gx).sum() + (dv * gv).sum())
    assert abs(lhs - rhs) < 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    # the KL alone
    ge, gx, gv = hk.hand_vjp(x0, v0, ext, S, G, feq, cot_kl)
    lhs, rhs = float((hkl * cot_kl).sum()), float((de * ge).sum() + (dx * gx).sum() + (dv * gv).sum())
    assert abs(lhs - rhs) < 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_kl_jvp_entries_are_declared_exported_and_typed():
    from ocplasma_amd import _abi, _build
    with open(os.path.join(ROOT, "include", "picstep.h")) as f:
        flat = re.sub(r"\s+", " ", f.read())
    m = re.search(r"int pic_phase_kl_smooth_jvp\(([^)]*)\);", flat)
    assert m, "pic_phase_kl_smooth_jvp is not declared in include/picstep.h"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 7
    m = re.search(r"int pic_tape_tangent_kl\(([^)]*)\);", flat)
    assert m, "pic_tape_tangent_kl is not declared in include/picstep.h"
    args = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert len(args) == 12 and args[-1] == "double* d_kl"
    # the arguments of pic_tape_tangent, then d_kl
    plain = re.search(r"int pic_tape_tangent\(([^)]*)\);", flat).group(1)
    assert [a.strip() for a in plain.split(",")] == args[:-1]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _abi.SIGNATURES["pic_phase_kl_smooth_jvp"] == [vp, ctypes.POINTER(_abi.PicPhaseSpec), ci, vp, vp, ci, vp]
    assert _abi.SIGNATURES["pic_tape_tangent_kl"] == _abi.SIGNATURES["pic_tape_tangent"] + [vp]
    lib = ctypes.CDLL(_build.build_library())
    for name in ("pic_phase_kl_smooth_jvp", "pic_tape_tangent_kl"):
        assert hasattr(lib, name), name
    assert "#define PICSTEP_ABI_VERSION 5" in flat and lib.pic_abi_version() == 5 == _abi.ABI_VERSION
    assert ctypes.sizeof(_abi.PicTapeInfo) == 56


def test_python_entries_take_the_kl_tangent():
    import inspect
    from ocplasma_amd.env.batched import BatchedPIC
    p = inspect.signature(BatchedPIC.tangent).parameters
    assert "kl" in p and p["kl"].default is False
    p = inspect.signature(BatchedPIC.kl_smooth_jvp).parameters
    assert list(p)[1:] == ["feq", "vmin", "vmax", "d_x", "d_v"]
