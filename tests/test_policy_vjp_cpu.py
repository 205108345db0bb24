"""The policy's vector-Jacobian product without a GPU: the NumPy restatement of its arithmetic
(tests/hp_mlp_policy_vjp.py) against torch autograd of the float64 twin (MLPPolicy.to_torch) and against central differences, the
declarations and bindings of the new entries, the Python layer, and the new kernels' resource report."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import hp_mlp_policy as hm
import hp_mlp_policy_vjp as hv
from conftest import ROOT

E, MO = 3, 2
WIDTHS = hm.stacks(MO)[1]             # [4, 37, 5, 4]
KINDS = [("tanh", False), ("relu", False), ("tanh", True), ("relu", True)]


def _policy(widths, activation, params, **kw):
    from ocplasma_amd.control.policy import MLPPolicy
    return MLPPolicy(widths, activation, params, widths[0] // 2, **kw)


def _case(activation, squash, obs_scale=None, widths=WIDTHS):
    return hv.vjp_case(E, widths[0] // 2, widths, activation, squash, seed=4, obs_scale=obs_scale)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("activation,squash", KINDS)
def test_restatement_agrees_with_autograd_of_the_twin(activation, squash, scaled):
    """The twin sums in another order (a BLAS product): agreement to a few hundred ulp of the largest entry, not bits."""
    import torch
    sc = np.linspace(0.5, 3.0, WIDTHS[0]) if scaled else None
    c = _case(activation, squash, sc)
    pol = _policy(WIDTHS, activation, c["params"], squash=squash, action_scale=c["action_scale"], obs_scale=sc)
    g_env, g_obs, g_pre = hv.vjp(**c)
    module = pol.to_torch()
    obs = torch.tensor(c["obs"], requires_grad=True)
    a = pol.torch_actions(module, obs)
    a.backward(torch.as_tensor(c["cot"]))
    g_twin = pol.pack([(module[2 * l].weight.grad.numpy(), module[2 * l].bias.grad.numpy()) for l in range(len(WIDTHS) - 1)])
    assert _rel(hv.sum_envs(g_env), g_twin) < 1e-13
    assert _rel(g_obs, obs.grad.numpy()) < 1e-13
    # u-bar against autograd of the squash alone
    u = torch.tensor(c["pre"], requires_grad=True)
    (c["action_scale"] * torch.tanh(u) if squash else u).backward(torch.as_tensor(c["cot"]))
    assert _rel(g_pre, u.grad.numpy()) < 1e-13


@pytest.mark.parametrize("activation,squash", KINDS)
def test_restatement_agrees_with_central_differences(activation, squash):
    """J = sum(cot * actions) as a function of the parameters and of the observation: central differences of the float64 forward
    with step 1e-6 are good to ~1e-9 of the gradient's scale (relu: away from a kink with this seed's margins)."""
    c = _case(activation, squash, np.linspace(0.5, 3.0, WIDTHS[0]))
    fw = {k: v for k, v in c.items() if k not in ("cot", "pre")}
    g_env, g_obs, _ = hv.vjp(**c)
    g = hv.sum_envs(g_env)
    J = lambda **kw: float(np.sum(c["cot"] * hm.forward(**{**fw, **kw})[1]))  # noqa: E731
    rng = np.random.default_rng(1)
    h = 1e-6
    for _ in range(4):
        d = rng.normal(size=c["params"].shape)
        fd = (J(params=c["params"] + h * d) - J(params=c["params"] - h * d)) / (2 * h)
        assert abs(fd - float(np.sum(g * d))) <= 1e-7 * max(1.0, abs(fd)), (fd, float(np.sum(g * d)))
        d = rng.normal(size=c["obs"].shape)
        fd = (J(obs=c["obs"] + h * d) - J(obs=c["obs"] - h * d)) / (2 * h)
        assert abs(fd - float(np.sum(g_obs * d))) <= 1e-7 * max(1.0, abs(fd)), (fd, float(np.sum(g_obs * d)))


def test_per_environment_rows_and_the_order_of_the_sums():
    c = hv.vjp_case(E, MO, WIDTHS, "tanh", True, seed=2, per_env=True)
    g_env, g_obs, g_pre = hv.vjp(**c)
    for e in range(E):
        one = {**c, "params": c["params"][e], "obs": c["obs"][e:e + 1], "cot": c["cot"][e:e + 1], "pre": c["pre"][e:e + 1]}
        ge, go, gu = hv.vjp(**one)
        assert np.array_equal(ge[0], g_env[e]) and np.array_equal(go[0], g_obs[e]) and np.array_equal(gu[0], g_pre[e])
    assert np.array_equal(hv.sum_envs(g_env), (g_env[0] + g_env[1]) + g_env[2])
    assert np.array_equal(hv.accumulate([g_env[2], g_env[1], g_env[0]]), (g_env[2] + g_env[1]) + g_env[0])


def test_floor_is_small_and_positive():
    f = hv.floor([_case("tanh", True), _case("relu", True)])
    assert 0.0 < f < 1e-13


def test_unpack_grad_round_trips_with_pack():
    from ocplasma_amd.control.policy import MLPPolicy
    pol = _policy(WIDTHS, "tanh", hm.make_params(WIDTHS, 1))
    g = np.random.default_rng(3).normal(size=pol.n_params)
    layers = pol.unpack_grad(g)
    assert [(W.shape, b.shape) for W, b in layers] == [((37, 4), (37,)), ((5, 37), (5,)), ((4, 5), (4,))]
    assert np.array_equal(MLPPolicy.pack(layers), g)
    module = pol.to_torch()
    for l, (W, b) in enumerate(layers):
        assert tuple(module[2 * l].weight.shape) == W.shape and tuple(module[2 * l].bias.shape) == b.shape
    ge = np.random.default_rng(4).normal(size=(E, pol.n_params))
    assert [W.shape for W, _ in pol.unpack_grad(ge)] == [(E, 37, 4), (E, 5, 37), (E, 4, 5)]
    with pytest.raises(ValueError):
        pol.unpack_grad(g[:-1])


DECLS = [
    "int pic_policy_vjp(pic_handle* h, const pic_policy* p, const double* obs, const double* pre, const double* cot_actions, "
    "int mem_kind, double* g_params, double* g_obs, double* g_pre);",
    "int pic_tape_step_policy(pic_handle* h, const pic_policy* p, const double* noise, const double* std, int mem_kind, int nsteps, "
    "double* obs_out, double* pre_out, double* actions_out, double* hist);",
    "int pic_tape_backward_policy(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, "
    "const double* cot_actions, const double* cot_obs, int mem_kind, double* g_params, double* g_pre, double* g_obs, "
    "double* g_actions, void* g_x0, void* g_v0);",
    "int pic_tape_policy_grad(pic_handle* h, int mem_kind, double* g_params);",
]
NAMES = {"pic_policy_vjp": 9, "pic_tape_step_policy": 10, "pic_tape_backward_policy": 13, "pic_tape_policy_grad": 3}


def test_entries_are_declared_bound_and_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for d in DECLS:
        assert d in flat, d
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    for name, n in NAMES.items():
        assert len(_abi.SIGNATURES[name]) == n, name       # (the arguments of the C prototypes above, the handle included)
        assert callable(getattr(_abi.Handle, name[4:])), name
    lib = ctypes.CDLL(_build.build_library())
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION


def test_new_kernels_are_scratch_free_and_within_lds():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    mine = {k: v for k, v in res.items() if "policy_vjp_kernel" in k or "policy_grad_reduce_kernel" in k}
    assert len(mine) == 2, sorted(mine)
    for k, v in mine.items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)
    vjp = next(v for k, v in mine.items() if "policy_vjp_kernel" in k)
    assert vjp["lds_bytes_per_block"] <= (5 * 256 + 2 * 256) * 8       # every layer's activations and two delta vectors
    assert any("policy_kernel" in k for k in res)                      # (the forward keeps its entry)


def test_python_layer_exists():
    from ocplasma_amd.control.policy import MLPPolicy
    from ocplasma_amd.env import grad
    from ocplasma_amd.env.batched import BatchedPIC
    assert list(inspect.signature(grad.rollout_mlp).parameters) == ["env", "policy", "params", "T", "noise", "std",
                                                                     "checkpoint_every", "kl"]
    p = inspect.signature(BatchedPIC.tape_step_policy).parameters
    assert list(p)[1:5] == ["policy", "nsteps", "noise", "std"]
    p = inspect.signature(BatchedPIC.backward_policy).parameters
    for k in ("d_KE", "d_PE", "d_PE_reward", "d_x", "d_v", "d_actions", "d_obs", "d_KL", "d_moments"):
        assert k in p, k
    assert callable(BatchedPIC.policy_vjp) and callable(BatchedPIC.tape_policy_grad) and callable(MLPPolicy.unpack_grad)
    assert list(inspect.signature(BatchedPIC.step_policy).parameters) == ["self", "policy", "nsteps", "noise", "std", "history",
                                                                         "on_device"]
