"""The closed loop under a generic torch policy without a GPU: the restatement (tests/hp_policy.py) with the
linear policy G0 against the gain law's restatement, its autograd gradient against central differences for an MLP on modes and
a DeepSets state policy, and the C declarations of the walk."""
import ctypes
import os
import re

import numpy as np
import torch

import hp_adjoint as ha
import hp_feedback as hf
import hp_policy as hpp
from conftest import rel_err
from oracle import pic_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(seed, N=500, Ng=32):
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x0, v0 = po.synthetic_bump_on_tail(N, S.L, seed=seed)
    return S, torch.as_tensor(np.asarray(x0, dtype=np.float64)), torch.as_tensor(np.asarray(v0, dtype=np.float64))


def test_linear_policy_reproduces_the_gain_law_restatement():
    S, x0, v0 = _setup(1)
    M, T = 3, 6
    G = torch.as_tensor(hf.g0(M))
    with torch.no_grad():
        hist, acts, obs = hpp.rollout(x0, v0, lambda m: G @ m, S, T, M)
        xT, vT, hist_f, modes_f, acts_f = hf.rollout(x0, v0, G, S, T, M)
    assert rel_err(hist.numpy(), hist_f.numpy()) <= 1e-15
    assert rel_err(acts.numpy(), acts_f.numpy()) <= 1e-15
    assert rel_err(torch.stack(obs[:T]).numpy(), modes_f.numpy()) <= 1e-15


def _fd_check(S, x0, v0, policy, params, T, M, observe, obs_modes=None, seed=0):
    rng = np.random.default_rng(seed)
    w_hist = rng.standard_normal((T, 3))
    w_obs = rng.standard_normal(2 * (obs_modes or M)) if observe == "modes" else None

    def J(p):
        hist, acts, obs = hpp.rollout(x0, v0, lambda o: policy(p, o), S, T, M, observe, obs_modes)
        return hpp.loss_terms(hist, acts, obs, w_hist, 0.05, w_obs)
    leaves = {k: t.clone().requires_grad_(True) for k, t in params.items()}
    grads = torch.autograd.grad(J(leaves), list(leaves.values()))
    d = {k: torch.as_tensor(rng.standard_normal(t.shape)) for k, t in params.items()}
    ad = float(sum((g * d[k]).sum() for g, k in zip(grads, leaves)))
    h = 1e-6
    with torch.no_grad():
        fd = (float(J({k: t + h * d[k] for k, t in params.items()})) - float(J({k: t - h * d[k] for k, t in params.items()}))) / (2 * h)
    assert abs(ad - fd) < 1e-5 * max(abs(fd), 1e-3), (ad, fd)


def test_mlp_on_modes_autograd_matches_central_differences():
    S, x0, v0 = _setup(3)
    M, Mo, T = 2, 4, 5
    p = hpp.mlp_params(2 * Mo, 2 * M, 8, seed=1)
    _fd_check(S, x0, v0, hpp.mlp_modes, p, T, M, "modes", Mo, seed=2)


def test_deepsets_state_policy_autograd_matches_central_differences():
    S, x0, v0 = _setup(4)
    M, T = 2, 4
    p = hpp.deepsets_params(2 * M, 8, seed=3)
    _fd_check(S, x0, v0, lambda q, o: hpp.deepsets_state(q, o, S.L), p, T, M, "state", seed=5)


def test_batched_policies_match_their_per_environment_slices():
    """The leading-axis convention the GPU tests rely on: p[e] applied to o[e] is row e of the batched call."""
    E, Mo, M, N = 3, 3, 2, 50
    g = torch.Generator().manual_seed(0)
    pm = hpp.mlp_params(2 * Mo, 2 * M, 5, lead=(E,), seed=1)
    m = torch.randn(E, 2 * Mo, generator=g, dtype=torch.float64)
    a = hpp.mlp_modes(pm, m)
    for e in range(E):
        assert torch.equal(a[e], hpp.mlp_modes({k: t[e] for k, t in pm.items()}, m[e]))
    ps = hpp.deepsets_params(2 * M, 5, lead=(E,), seed=2)
    x, v = torch.rand(E, N, generator=g, dtype=torch.float64) * 50, torch.randn(E, N, generator=g, dtype=torch.float64)
    a = hpp.deepsets_state(ps, (x, v), 50.0)
    for e in range(E):
        assert rel_err(a[e].numpy(), hpp.deepsets_state({k: t[e] for k, t in ps.items()}, (x[e], v[e]), 50.0).numpy()) < 1e-15


def test_walk_entries_are_declared_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int pic_tape_walk_begin(pic_handle* h, int obs_modes, int mem_kind);" in flat
    assert ("int pic_tape_walk_step(pic_handle* h, const double* cot_energies, const void* cot_x, const void* cot_v, "
            "const double* cot_modes, int mem_kind, double* g_ext, double* g_actions, int64_t* step);") in flat
    assert ("int pic_tape_walk_end(pic_handle* h, const void* cot_x0, const void* cot_v0, const double* cot_modes0, int mem_kind, "
            "void* g_x0, void* g_v0);") in flat
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _abi.SIGNATURES["pic_tape_walk_begin"] == [vp, ci, ci]
    assert _abi.SIGNATURES["pic_tape_walk_step"] == [vp, vp, vp, vp, vp, ci, vp, vp, ctypes.POINTER(ctypes.c_int64)]
    assert _abi.SIGNATURES["pic_tape_walk_end"] == [vp, vp, vp, vp, ci, vp, vp]
    lib = ctypes.CDLL(_build.build_library())
    for name in ("pic_tape_walk_begin", "pic_tape_walk_step", "pic_tape_walk_end"):
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_rollout_policy_is_exported():
    from ocplasma_amd.env import grad
    from ocplasma_amd.env.batched import BatchedPIC
    assert callable(grad.rollout_policy) and callable(BatchedPIC.walk)
