"""Forward mode through closed loops without a GPU: the hand-written closed-loop tangent equations
(tests/hp_tangent_walk.py) against torch forward-mode AD of the restatements of the gain law and of a policy loop, the
declarations and bindings of the new entries, and the new kernels' resource report."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import hp_adjoint as ha
import hp_feedback as hf
import hp_policy as hpol
import hp_tangent_walk as hw
from conftest import ROOT, rel_err
from oracle import pic_oracle as po

N, NG, T, M = 400, 32, 4, 3
L = 50.0
SEED = 5
NODE_EPS = 1e-9                   # no sub-stage position within 1e-9 cells of a node


def _problem():
    S = ha.Setup(N, NG, L, 1.0, 0.1)
    x0, v0 = po.synthetic_bump_on_tail(N, L, seed=SEED)
    rng = np.random.default_rng(SEED)
    return S, np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64), rng


def _np_params(p):
    return {k: a.numpy() for k, a in p.items()}


def test_gain_law_hand_jvp_matches_torch_forward_mode():
    S, x0, v0, rng = _problem()
    G = hf.g0(M) + 0.3 * rng.standard_normal((2 * M, 2 * M))
    dG, dx, dv = rng.standard_normal((2 * M, 2 * M)), rng.standard_normal(N), rng.standard_normal(N)
    for u in ({"dG": dG}, {"d_x0": dx}, {"d_v0": dv}, {"dG": dG, "d_x0": dx, "d_v0": dv}):
        hh, hm, hact, hx, hv, _, exts = hw.hand_feedback_jvp(x0, v0, G, S, T, M, **u)
        assert hw.node_distance(x0, v0, exts, S) > NODE_EPS
        th, tm, tact, tx, tv = hw.torch_feedback_jvp(x0, v0, G, S, T, M, **u)
        for got, want in ((hh, th), (hm, tm), (hact, tact), (hx, tx), (hv, tv)):
            assert rel_err(got, want) < 1e-10, (sorted(u), rel_err(got, want))


def test_gain_law_injection_is_the_derivative_along_a_second_gain():
    """d_actions_t = dG2 m_t injected next to dG1 gives the tangent along dG1 + dG2 (how tapes with several gains are served)."""
    S, x0, v0, rng = _problem()
    G = hf.g0(M) + 0.3 * rng.standard_normal((2 * M, 2 * M))
    dG1, dG2 = rng.standard_normal((2 * M, 2 * M)), rng.standard_normal((2 * M, 2 * M))
    import torch
    with torch.no_grad():
        modes = hf.rollout(torch.as_tensor(x0), torch.as_tensor(v0), torch.as_tensor(G), S, T, M)[3].numpy()
    inj = modes @ dG2.T
    got = hw.hand_feedback_jvp(x0, v0, G, S, T, M, dG=dG1, d_actions=inj)
    want = hw.hand_feedback_jvp(x0, v0, G, S, T, M, dG=dG1 + dG2)
    for g, w in zip(got[:5], want[:5]):
        assert rel_err(g, w) < 1e-12


@pytest.mark.parametrize("observe", ["modes", "state"])
def test_policy_hand_jvp_matches_torch_forward_mode(observe):
    S, x0, v0, rng = _problem()
    if observe == "modes":
        p = hpol.mlp_params(2 * M, 2 * M, 8, seed=2)
        fn_t, fn_np, fn_jvp = hpol.mlp_modes, hw.mlp_modes_np, hw.mlp_modes_jvp
    else:
        p = hpol.deepsets_params(2 * M, 8, seed=2)
        fn_t = lambda q, o: hpol.deepsets_state(q, o, L)                             # noqa: E731
        fn_np = lambda q, o: hw.deepsets_state_np(q, o, L)                           # noqa: E731
        fn_jvp = lambda q, o, dq, do: hw.deepsets_state_jvp(q, o, L, dq, do)         # noqa: E731
    pn = _np_params(p)
    dp = {k: rng.standard_normal(a.shape) for k, a in pn.items()}
    dx, dv = rng.standard_normal(N), rng.standard_normal(N)
    hh, hact, _, _, exts = hw.hand_policy_jvp(x0, v0, fn_np, fn_jvp, pn, dp, S, T, M, observe, d_x0=dx, d_v0=dv)
    assert hw.node_distance(x0, v0, exts, S) > NODE_EPS
    th, tact = hw.torch_policy_jvp(x0, v0, fn_t, p, dp, S, T, M, observe, d_x0=dx, d_v0=dv)
    assert rel_err(hh, th) < 1e-10, rel_err(hh, th)
    assert rel_err(hact, tact) < 1e-10, rel_err(hact, tact)


# ---- declarations, bindings, build -------------------------------------------------------------------------------------------------
DECLS = (
    "int pic_tape_tangent_walk_begin(pic_handle* h, int K, int obs_modes, const void* d_x0, const void* d_v0, const double* d_gain, "
    "int mem_kind, double* d_modes0);",
    "int pic_tape_tangent_walk_step(pic_handle* h, const double* d_ext, const double* d_actions, int mem_kind, double* d_energies, "
    "double* d_modes, double* d_actions_out, void* d_x, void* d_v, double* d_E_mesh, int64_t* step);",
    "int pic_tape_tangent_walk_end(pic_handle* h, int mem_kind, void* d_x, void* d_v);",
    "int pic_tape_tangent_feedback(pic_handle* h, int K, const double* d_gain, const void* d_x0, const void* d_v0, "
    "const double* d_actions, int mem_kind, double* d_hist, double* d_modes, double* d_actions_out, void* d_x, void* d_v, "
    "double* d_E_mesh);",
)
NAMES = {"pic_tape_tangent_walk_begin": 8, "pic_tape_tangent_walk_step": 11, "pic_tape_tangent_walk_end": 4,
         "pic_tape_tangent_feedback": 13}


def test_entries_are_declared_bound_and_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for d in DECLS:
        assert d in flat, d
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    for name, n in NAMES.items():
        assert len(_abi.SIGNATURES[name]) == n, name       # (the arguments of the C prototypes above, the handle included)
    assert len(_abi.SIGNATURES["pic_tape_tangent"]) == 11
    for name in NAMES:
        assert callable(getattr(_abi.Handle, name[4:])), name
    lib = ctypes.CDLL(_build.build_library())
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_new_kernels_are_scratch_free():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    want = {"tangent_law_kernel": 1, "tangent_start_deposit_kernel": 3, "tangent_x_max_kernel": 1, "tangent_action_kernel": 1}
    for name, count in want.items():
        mine = {k: r for k, r in res.items() if name in k}
        assert len(mine) == count, (name, sorted(mine))
        for k, r in mine.items():
            assert r["scratch_bytes_per_lane"] == 0, (k, r)


def test_python_layer_exists():
    from ocplasma_amd.env import grad
    from ocplasma_amd.env.batched import BatchedPIC, TangentWalk
    p = inspect.signature(BatchedPIC.tangent_walk).parameters
    assert [k for k in p][1:] == ["K", "obs_modes", "d_x0", "d_v0", "d_gain", "on_device"]
    assert all(p[k].default is None for k in ("K", "obs_modes", "d_x0", "d_v0", "d_gain")) and p["on_device"].default is False
    p = inspect.signature(TangentWalk.step).parameters
    assert [k for k in p][1:] == ["d_actions", "d_ext", "state", "fields"] and callable(TangentWalk.end)
    p = inspect.signature(BatchedPIC.tangent_feedback).parameters
    assert [k for k in p][1:] == ["d_gain", "d_x0", "d_v0", "d_actions", "fields"]
    p = inspect.signature(grad.rollout_policy_jvp).parameters
    assert [k for k in p] == ["env", "fn", "params", "d_params", "T", "observe", "obs_modes", "d_x0", "d_v0", "checkpoint_every"]
    assert callable(grad._RolloutFeedback.jvp)
    with pytest.raises(ValueError, match="moments"):
        grad.rollout_policy_jvp(type("E", (), {"max_mode": 3})(), None, {}, [{}], 2, observe="moments")
