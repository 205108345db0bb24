"""CPU checks of the MLP policy's host layer: the NumPy restatement of the device's arithmetic against its
extended-precision twin and against torch's own forward, the packing helpers of control/policy.py, and the C ABI's surface."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import hp_mlp_policy as hm
from ocplasma_amd import _abi, _build
from ocplasma_amd.control.policy import MLPPolicy, param_count


@pytest.fixture(scope="module")
def floor():
    """100 x the largest float64 - longdouble difference of the restatement over the GPU test's tanh cases: its tolerance."""
    return 100 * hm.floor(hm.tanh_cases())


def test_restatement_matches_its_longdouble_twin(floor):
    assert 0 < floor < 1e-11, floor
    # a relu network without squash has no transcendental: float64 and longdouble agree to the sums' rounding alone
    c = hm.eval_case(3, 5, hm.stacks(5)[2], "relu", False)
    assert hm.floor([c]) <= floor / 100


def test_restatement_sums_in_ascending_k():
    """The order is part of the contract: a sum whose value depends on it comes out as the ascending loop gives it."""
    widths = [4, 1]
    params = np.array([1e16, 1.0, -1e16, 1.0, 0.0])            # W = [1e16, 1, -1e16, 1], b = 0
    u, a = hm.forward(widths, "relu", params, np.ones((1, 4)))
    assert u[0, 0] == 1.0 and a[0, 0] == 1.0                   # ((0 + 1e16) + 1) - 1e16 + 1 = 1; pairwise or sorted sums give 2 or 0


def test_relu_gives_positive_zero():
    u, _ = hm.forward([2, 2, 1], "relu", np.array([-1.0, 0, 0, -1.0, 0, 0, 1.0, 1.0, 0.0]), np.ones((1, 2)))
    assert u[0, 0] == 0.0 and not np.signbit(u[0, 0])


@pytest.mark.parametrize("widths", [[4, 4], [10, 37, 5, 4], [6, 64, 64, 6], [4, 8, 8, 8, 4]])
def test_pack_unpack_round_trip(widths):
    p = hm.make_params(widths, 3)
    pol = MLPPolicy(widths, "tanh", p, widths[0] // 2)
    layers = pol.unpack()
    assert [W.shape for W, _ in layers] == [(widths[l + 1], widths[l]) for l in range(len(widths) - 1)]
    assert np.array_equal(MLPPolicy.pack(layers), p) and pol.n_params == param_count(widths) == hm.param_count(widths)
    for (W, b), (Wh, bh) in zip(layers, hm.layers_of(widths, p)):
        assert np.array_equal(W, Wh) and np.array_equal(b, bh)
    again = MLPPolicy.from_layers(layers, "tanh", widths[0] // 2)
    assert again.widths == widths and np.array_equal(again.params, p)


@pytest.mark.parametrize("activation,squash", [("tanh", False), ("relu", False), ("tanh", True), ("relu", True)])
def test_torch_round_trip_and_forward(floor, activation, squash):
    import torch
    import torch.nn as nn
    torch.manual_seed(4)
    act = nn.Tanh if activation == "tanh" else nn.ReLU
    mods = [nn.Linear(6, 64), act(), nn.Linear(64, 64), act(), nn.Linear(64, 6)] + ([nn.Tanh()] if squash else [])
    net = nn.Sequential(*mods).double()
    pol = MLPPolicy.from_torch(net, obs_modes=3, action_scale=1.25)
    assert pol.widths == [6, 64, 64, 6] and pol.activation == activation and pol.squash == squash
    twin = pol.to_torch()
    assert [type(m) for m in twin] == [type(m) for m in net]
    for m, t in zip(net, twin):
        if isinstance(m, nn.Linear):
            assert t.weight.dtype == torch.float64 and torch.equal(m.weight, t.weight) and torch.equal(m.bias, t.bias)
    assert np.array_equal(MLPPolicy.from_torch(twin, 3).params, pol.params)
    obs = 0.5 * np.random.default_rng(5).normal(size=(7, 6))
    _, a = hm.forward(pol.widths, activation, pol.params, obs, squash=squash, action_scale=pol.action_scale)
    with torch.no_grad():
        ref = pol.torch_actions(net, torch.from_numpy(obs)).numpy()
    assert np.max(np.abs(a - ref)) <= floor, (np.max(np.abs(a - ref)), floor)


def test_stack_makes_a_per_environment_policy():
    widths = [4, 5, 4]
    ps = [MLPPolicy(widths, "relu", hm.make_params(widths, s), 2) for s in range(3)]
    st = MLPPolicy.stack(ps)
    assert st.per_env and st.params.shape == (3, param_count(widths))
    for e, p in enumerate(ps):
        assert np.array_equal(st.params[e], p.params)
    W, b = st.unpack()[1]
    assert W.shape == (3, 4, 5) and b.shape == (3, 4)
    with pytest.raises(ValueError):
        MLPPolicy.stack([ps[0], MLPPolicy(widths, "tanh", ps[1].params, 2)])
    with pytest.raises(ValueError):
        st.to_torch()


def test_bad_policies_are_rejected():
    ok = hm.make_params([4, 5, 4], 0)
    with pytest.raises(ValueError, match="activation"):
        MLPPolicy([4, 5, 4], "gelu", ok, 2)
    with pytest.raises(ValueError, match="chain"):
        MLPPolicy([6, 5, 4], "tanh", hm.make_params([6, 5, 4], 0), 2)             # 2 obs_modes = 4 != 6
    with pytest.raises(ValueError, match="chain"):
        MLPPolicy.pack([(np.zeros((5, 4)), np.zeros(5)), (np.zeros((4, 6)), np.zeros(4))])
    with pytest.raises(ValueError, match="params"):
        MLPPolicy([4, 5, 4], "tanh", ok[:-1], 2)
    with pytest.raises(ValueError):
        MLPPolicy([4, 300, 4], "tanh", hm.make_params([4, 300, 4], 0), 2)
    with pytest.raises(ValueError):
        MLPPolicy([4, 4, 4, 4, 4, 4], "tanh", hm.make_params([4, 4, 4, 4, 4, 4], 0), 2)
    import torch.nn as nn
    with pytest.raises(ValueError):
        MLPPolicy.from_torch(nn.Sequential(nn.Linear(4, 5), nn.Sigmoid(), nn.Linear(5, 4)), 2)
    with pytest.raises(ValueError):
        MLPPolicy.from_torch(nn.Sequential(nn.Linear(4, 5), nn.Tanh(), nn.Linear(5, 5), nn.ReLU(), nn.Linear(5, 4)), 2)


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    for name in ("pic_policy_eval", "pic_step_policy"):
        assert re.search(r"^int\s+" + name + r"\s*\(pic_handle\* h, const pic_policy\* p,", hdr, re.M), name
        assert name in _abi.SIGNATURES
    assert "additive to ABI 5" in hdr[hdr.index("MLP policy"):hdr.index("typedef struct pic_policy")]
    lib = ctypes.CDLL(_build.build_library())
    assert hasattr(lib, "pic_policy_eval") and hasattr(lib, "pic_step_policy") and lib.pic_abi_version() == 5
    # the struct's fields, in the header's order and C's layout
    body = hdr[hdr.index("typedef struct pic_policy {"):hdr.index("} pic_policy;")]
    fields = re.findall(r"^\s*(?:int|double|const double\*)\s+(\w+)(?:\[5\])?;", body, re.M)
    assert fields == [f[0] for f in _abi.PicPolicy._fields_], fields
    assert ctypes.sizeof(_abi.PicPolicy) == 10 * 4 + 8 + 2 * 8 and _abi.PicPolicy.action_scale.offset == 40
    assert re.search(r"#define PIC_ACT_TANH 0\n#define PIC_ACT_RELU 1", hdr) and _abi.ACTIVATIONS == {"tanh": 0, "relu": 1}
    rep = __import__("json").load(open(_build.RESOURCES))
    mine = [v for k, v in rep.items() if "policy_kernel" in k]
    assert len(mine) == 1 and mine[0]["scratch_bytes_per_lane"] == 0, mine
