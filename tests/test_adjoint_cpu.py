"""The adjoint's oracle without a GPU: the torch restatement of the step (tests/hp_adjoint.py) against the
reference's goldens, its autograd gradient against finite differences, and the hand-written reverse equations the kernels
implement against autograd."""
import numpy as np
import pytest
import torch

import hp_adjoint as ha
from conftest import load_golden, rel_err
from oracle import pic_oracle as po


def _golden_rollout(name, K, ext):
    g = load_golden(name)
    N, Ng = int(g["N"]), int(g["Ng"])
    S = ha.Setup(N, Ng, float(g["L"]), float(g["n0"]), float(g["dt"]))
    mm = g["actions"].shape[1] // 2 if "actions" in g else 0
    e = np.zeros((K, Ng))
    if ext:
        for k in range(K):
            a = g["actions"][k]
            e[k] = po.actuator_field(S.L, Ng, mm, a[:mm], a[mm:]).ravel()
    x, v = torch.as_tensor(g["x_init"].ravel()), torch.as_tensor(g["v_init"].ravel())
    hist, marks = [], {}
    with torch.no_grad():
        for k in range(1, K + 1):
            x, v, ke, pe, per, M = ha.step(x, v, torch.as_tensor(e[k - 1]), S)
            hist.append((float(ke), float(pe), float(per)))
            marks[k] = (x.numpy().copy(), v.numpy().copy(), M.numpy().copy())
    return g, marks, np.array(hist)


def test_restatement_matches_golden_two_stream():
    g, marks, hist = _golden_rollout("g5_two_stream_N5000_Ng250", 10, False)
    for k in (1, 10):
        x, v, Em = marks[k]
        assert rel_err(x, g[f"x_{k}"]) < 1e-11 and rel_err(v, g[f"v_{k}"]) < 1e-11
        assert rel_err(Em, g[f"E_mesh_{k}"]) < 1e-10
    assert rel_err(hist[:, 0], g["KE"][1:11]) < 1e-13
    assert rel_err(hist[:, 1], g["PE"][1:11]) < 1e-10


@pytest.mark.parametrize("name", ["g4_two_stream_ext_N3000_Ng200", "g4_bump_on_tail_ext_N4000_Ng256"])
def test_restatement_matches_golden_with_external_field(name):
    g, marks, hist = _golden_rollout(name, 20, True)
    for k in (1, 20):
        x, v, Em = marks[k]
        assert rel_err(x, g[f"x_{k}"]) < 1e-11 and rel_err(v, g[f"v_{k}"]) < 1e-11
        assert rel_err(Em, g[f"E_mesh_{k}"]) < 1e-10
    assert rel_err(hist[:, 0], g["KE"][1:21]) < 1e-13
    assert rel_err(hist[:, 1], g["PE"][1:21]) < 1e-10


def _problem(N, Ng, T, seed):
    rng = np.random.default_rng(seed)
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x0, v0 = po.synthetic_bump_on_tail(N, S.L, seed=seed)
    ext = 0.05 * rng.standard_normal((T, Ng))
    cot = rng.standard_normal((T, 3))
    cx, cv = rng.standard_normal(N), rng.standard_normal(N)
    return S, np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64), ext, cot, cx, cv, rng


@pytest.mark.parametrize("N,Ng,T", [(2000, 64, 3), (1000, 32, 5)])
def test_autograd_matches_central_differences(N, Ng, T):
    S, x0, v0, ext, cot, cx, cv, rng = _problem(N, Ng, T, 11)
    ge, gx, gv = ha.autograd_vjp(x0, v0, ext, S, cot, cx, cv)
    eps = 1e-6
    for _ in range(3):
        de, dxx, dvv = rng.standard_normal(ext.shape), rng.standard_normal(N), rng.standard_normal(N)
        Jp = ha.objective(x0 + eps * dxx, v0 + eps * dvv, ext + eps * de, S, cot, cx, cv)
        Jm = ha.objective(x0 - eps * dxx, v0 - eps * dvv, ext - eps * de, S, cot, cx, cv)
        fd = (Jp - Jm) / (2 * eps)
        an = float((ge * de).sum() + (gx * dxx).sum() + (gv * dvv).sum())
        assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-12), (fd, an)


@pytest.mark.parametrize("N,Ng,T", [(2000, 64, 3), (3000, 250, 5)])
def test_hand_adjoint_matches_autograd(N, Ng, T):
    S, x0, v0, ext, cot, cx, cv, _ = _problem(N, Ng, T, 5)
    ge, gx, gv = ha.autograd_vjp(x0, v0, ext, S, cot, cx, cv)
    he, hx, hv = ha.hand_vjp(x0, v0, ext, S, cot, cx, cv)
    assert rel_err(he, ge) < 1e-10
    assert rel_err(hx, gx) < 1e-10
    assert rel_err(hv, gv) < 1e-10
    # energy cotangents alone (no final-state term): the refresh adjoint carries everything
    ge, gx, gv = ha.autograd_vjp(x0, v0, ext, S, cot)
    he, hx, hv = ha.hand_vjp(x0, v0, ext, S, cot)
    assert rel_err(he, ge) < 1e-10 and rel_err(hx, gx) < 1e-10 and rel_err(hv, gv) < 1e-10
