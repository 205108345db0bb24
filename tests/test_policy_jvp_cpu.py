"""The policy's Jacobian-vector product without a GPU: the NumPy restatement of its arithmetic
(tests/hp_mlp_policy_jvp.py) against torch.func.jvp of the float64 twin (MLPPolicy.to_torch), against central differences and, by
duality, against the VJP's restatement; the closed-loop hand equations with that JVP applied step by step against torch forward
mode of tests/hp_policy.py's rollout; the declarations and bindings of the new entries, the Python layer, and the new kernel's
resource report."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import hp_adjoint as ha
import hp_mlp_policy as hm
import hp_mlp_policy_jvp as hj
import hp_mlp_policy_vjp as hv
import hp_tangent_walk as hw
from conftest import ROOT, rel_err
from oracle import pic_oracle as po

E, MO = 3, 2
WIDTHS = hm.stacks(MO)[1]             # [4, 37, 5, 4]
KINDS = [("tanh", False), ("relu", False), ("tanh", True), ("relu", True)]


def _policy(widths, activation, params, **kw):
    from ocplasma_amd.control.policy import MLPPolicy
    return MLPPolicy(widths, activation, params, widths[0] // 2, **kw)


def _case(activation, squash, obs_scale=None, widths=WIDTHS, per_env=False):
    return hj.jvp_case(E, widths[0] // 2, widths, activation, squash, seed=4, obs_scale=obs_scale, per_env=per_env)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _forward_args(c):
    return {k: v for k, v in c.items() if k not in ("pre", "d_params", "d_obs", "d_pre")}


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("activation,squash", KINDS)
def test_restatement_agrees_with_forward_mode_of_the_twin(activation, squash, scaled):
    """The twin sums in another order (a BLAS product): agreement to a few hundred ulp of the largest entry, not bits."""
    import torch
    sc = np.linspace(0.5, 3.0, WIDTHS[0]) if scaled else None
    c = _case(activation, squash, sc)
    pol = _policy(WIDTHS, activation, c["params"], squash=squash, action_scale=c["action_scale"], obs_scale=sc)
    du, da = hj.jvp(**{**c, "d_pre": None})
    module = pol.to_torch()
    names = [n for n, _ in module.named_parameters()]
    params = {n: p.detach() for n, p in module.named_parameters()}
    dl = pol.unpack(c["d_params"])
    tangents = {}
    for l, (dW, db) in enumerate(dl):
        tangents[f"{2 * l}.weight"], tangents[f"{2 * l}.bias"] = torch.as_tensor(dW.copy()), torch.as_tensor(db.copy())
    assert sorted(tangents) == sorted(names)
    fn = lambda p, o: pol.torch_actions(lambda x: torch.func.functional_call(module, p, (x,)), o)  # noqa: E731
    got = torch.func.jvp(fn, (params, torch.as_tensor(c["obs"])), (tangents, torch.as_tensor(c["d_obs"])))[1].numpy()
    assert _rel(da, got) < 1e-13
    # the injection in front of the squash: da is linear in it with the squash's own derivative
    du2, da2 = hj.jvp(**c)
    assert np.array_equal(du2, du + c["d_pre"])
    u = torch.as_tensor(c["pre"])
    want = torch.func.jvp(lambda u: c["action_scale"] * torch.tanh(u) if squash else u, (u,), (torch.as_tensor(du2),))[1].numpy()
    assert _rel(da2, want) < 1e-13


@pytest.mark.parametrize("activation,squash", KINDS)
def test_restatement_agrees_with_central_differences(activation, squash):
    """Central differences of the float64 forward along (d_params, d_obs) with step 1e-6 are good to ~1e-9 of the tangent's scale
    (relu: away from a kink with this seed's margins)."""
    c = _case(activation, squash, np.linspace(0.5, 3.0, WIDTHS[0]))
    fw = _forward_args(c)
    _, da = hj.jvp(**{**c, "d_pre": None})
    h = 1e-6
    f = lambda s: hm.forward(**{**fw, "params": c["params"] + s * c["d_params"], "obs": c["obs"] + s * c["d_obs"]})[1]  # noqa: E731
    fd = (f(h) - f(-h)) / (2 * h)
    assert np.max(np.abs(fd - da)) <= 1e-7 * max(1.0, np.max(np.abs(da))), np.max(np.abs(fd - da))


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("activation,squash", KINDS)
def test_duality_with_the_vjp_restatement(activation, squash, per_env):
    """<c, J d> = <J^T c, d> over the parameters, the observation and pre, per environment."""
    c = _case(activation, squash, np.linspace(0.5, 3.0, WIDTHS[0]), per_env=per_env)
    cot = np.random.default_rng(8).normal(size=(E, WIDTHS[-1]))
    du, da = hj.jvp(**c)
    g_env, g_obs, g_pre = hv.vjp(cot=cot, **_forward_args(c), pre=c["pre"])
    dth = c["d_params"] if per_env else np.broadcast_to(c["d_params"], g_env.shape)
    lhs = (cot * da).sum(1)
    rhs = (g_env * dth).sum(1) + (g_obs * c["d_obs"]).sum(1) + (g_pre * c["d_pre"]).sum(1)
    assert np.max(np.abs(lhs - rhs)) <= 1e-12 * max(np.max(np.abs(lhs)), np.max(np.abs(rhs)))


def test_missing_tangents_are_zeros_and_rows_are_the_environments_own():
    c = _case("tanh", True, per_env=True)
    z = {**c, "d_params": np.zeros_like(c["d_params"]), "d_obs": np.zeros_like(c["d_obs"])}
    du0, da0 = hj.jvp(**{**c, "d_params": None, "d_obs": None})
    duz, daz = hj.jvp(**z)
    assert np.array_equal(du0, duz) and np.array_equal(da0, daz) and np.array_equal(du0, c["d_pre"])
    du, da = hj.jvp(**c)
    for e in range(E):
        one = {k: (v[e:e + 1] if k in ("obs", "pre", "d_obs", "d_pre") else v[e] if k in ("params", "d_params") else v)
               for k, v in c.items()}
        u1, a1 = hj.jvp(**one)
        assert np.array_equal(u1[0], du[e]) and np.array_equal(a1[0], da[e])


def test_floor_is_small_and_positive():
    f = hj.floor([_case("tanh", True), _case("relu", True), _case("tanh", False)])
    assert 0.0 < f < 1e-13


# ---- the closed loop --------------------------------------------------------------------------------------------------------------
N, NG, T, M = 400, 32, 4, hm.M
L = 50.0
NODE_EPS = 1e-9                   # no sub-stage position within 1e-9 cells of a node


def test_closed_loop_hand_jvp_matches_torch_forward_mode():
    """The restatement applied step by step inside the closed-loop tangent equations (hp_tangent_walk.hand_policy_jvp) against
    torch forward mode of hp_policy.rollout under the to_torch() twin, along the parameters, x_0 and v_0 together."""
    import torch
    Mo = 2
    widths = hm.stacks(Mo)[1]
    scale = np.full(2 * Mo, 8.0)
    pol = _policy(widths, "tanh", hm.make_params(widths, 5), squash=True, action_scale=1.25, obs_scale=scale)
    S = ha.Setup(N, NG, L, 1.0, 0.1)
    rng = np.random.default_rng(5)
    d_params, dx, dv = rng.standard_normal(pol.n_params), rng.standard_normal(N), rng.standard_normal(N)
    kw = dict(widths=widths, activation="tanh", squash=True, action_scale=1.25, obs_scale=scale)

    def fn(p, o):
        return hm.forward(params=p, obs=o[None], **kw)[1][0]

    def fn_jvp(p, o, dp, do):
        u = hm.forward(params=p, obs=o[None], **kw)[0]
        return hj.jvp(params=p, obs=o[None], pre=u, d_params=dp, d_obs=do[None], **kw)[1][0]

    module = pol.to_torch()
    names = [n for n, _ in module.named_parameters()]
    tp = {n: q.detach() for n, q in module.named_parameters()}
    dl = pol.unpack(d_params)
    tdp = {}
    for l, (dW, db) in enumerate(dl):
        tdp[f"{2 * l}.weight"], tdp[f"{2 * l}.bias"] = dW.copy(), db.copy()
    assert sorted(tdp) == sorted(names)
    fn_t = lambda p, o: pol.torch_actions(lambda x: torch.func.functional_call(module, p, (x,)), o)  # noqa: E731
    for seed in (5, 6, 7, 8):          # (a draw with a position on a node gets another seed, never another threshold)
        x0, v0 = (np.asarray(a, dtype=np.float64) for a in po.synthetic_bump_on_tail(N, L, seed=seed))
        hh, hact, _, _, exts = hw.hand_policy_jvp(x0, v0, fn, fn_jvp, np.asarray(pol.params), d_params, S, T, M, "modes", Mo,
                                                  d_x0=dx, d_v0=dv)
        if hw.node_distance(x0, v0, exts, S) > NODE_EPS:
            break
    assert hw.node_distance(x0, v0, exts, S) > NODE_EPS
    th, tact = hw.torch_policy_jvp(x0, v0, fn_t, tp, tdp, S, T, M, "modes", Mo, d_x0=dx, d_v0=dv)
    assert np.any(hact != 0.0)
    assert rel_err(hh, th) < 1e-10, rel_err(hh, th)
    assert rel_err(hact, tact) < 1e-10, rel_err(hact, tact)


# ---- declarations, bindings, build -------------------------------------------------------------------------------------------------
DECLS = [
    "int pic_policy_jvp(pic_handle* h, const pic_policy* p, const double* obs, const double* pre, int K, const double* d_params, "
    "const double* d_obs, const double* d_pre, int mem_kind, double* d_pre_out, double* d_actions_out);",
    "int pic_tape_tangent_policy(pic_handle* h, int K, const double* d_params, const double* d_pre, const double* d_actions, "
    "const void* d_x0, const void* d_v0, int mem_kind, double* d_hist, double* d_obs, double* d_pre_out, double* d_actions_out, "
    "void* d_x, void* d_v, double* d_E_mesh);",
]
NAMES = {"pic_policy_jvp": 11, "pic_tape_tangent_policy": 15}


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


def test_new_kernel_is_scratch_free_and_within_lds():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    mine = {k: v for k, v in res.items() if "policy_jvp_kernel" in k}
    assert len(mine) == 1, sorted(mine)
    (v,) = mine.values()
    assert v["scratch_bytes_per_lane"] == 0, v
    assert v["lds_bytes_per_block"] <= 4 * 256 * 8                     # two activation vectors and their two tangents
    # (the forward and the VJP keep their entries)
    assert sum("policy_vjp_kernel" in k for k in res) == 1 and any("policy_kernel" in k for k in res)


def test_python_layer_exists():
    from ocplasma_amd.control.policy import MLPPolicy
    from ocplasma_amd.env import grad
    from ocplasma_amd.env.batched import BatchedPIC
    p = inspect.signature(BatchedPIC.policy_jvp).parameters
    assert list(p)[1:] == ["policy", "obs", "pre", "d_params", "d_obs", "d_pre", "on_device"]
    assert all(p[k].default is None for k in ("pre", "d_params", "d_obs", "d_pre")) and p["on_device"].default is False
    p = inspect.signature(BatchedPIC.tangent_policy).parameters
    assert list(p)[1:] == ["d_params", "d_std", "noise", "d_pre", "d_actions", "d_x0", "d_v0", "fields", "on_device"]
    assert all(p[k].default is None for k in list(p)[1:8]) and p["fields"].default is False and p["on_device"].default is False
    assert callable(grad._RolloutMLP.jvp)
    pol = _policy(WIDTHS, "tanh", hm.make_params(WIDTHS, 1))
    d = np.random.default_rng(3).normal(size=pol.n_params)
    assert np.array_equal(pol.pack_tangent(pol.unpack(d)), d)
    layers = [(None, None)] * 3
    layers[1] = (np.ones((5, 37)), None)
    got = pol.unpack(pol.pack_tangent(layers))
    assert not got[0][0].any() and not got[2][1].any() and np.array_equal(got[1][0], np.ones((5, 37))) and not got[1][1].any()
    with pytest.raises(ValueError):
        pol.pack_tangent(layers[:2])
    with pytest.raises(ValueError):
        pol.pack_tangent([(np.ones((3, 3)), None)] * 3)
    assert callable(MLPPolicy.pack_tangent)
