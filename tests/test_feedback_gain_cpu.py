"""The gain law's oracle without a GPU: the closed-loop restatement (tests/hp_feedback.py) with G0 against the
reference's own feedback loop (G12), its autograd gradient against central differences, the hand-written law terms of the
reverse pass against autograd, and the C declarations of the new entries."""
import ctypes
import os
import re

import numpy as np
import torch

import hp_adjoint as ha
import hp_feedback as hf
from conftest import load_golden, rel_err
from oracle import pic_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_g0_restatement_follows_the_reference_feedback_loop():
    g = load_golden("g12_feedback_two_stream_N5000_Ng250")
    L, Ng, N, mm = float(g["L"]), int(g["Ng"]), int(g["N"]), int(g["max_mode"])
    S = ha.Setup(N, Ng, L, 1.0, float(g["dt"]))
    B = torch.as_tensor(hf.basis(L, Ng, mm))
    Jm = torch.as_tensor(hf.jacobian(Ng, mm))
    G0 = torch.as_tensor(hf.g0(mm))
    x, v = torch.as_tensor(g["x_init"].ravel()), torch.as_tensor(g["v_init"].ravel())
    with torch.no_grad():
        E = ha.field(ha.density(x, S), S)
        for k in range(1, 51):
            a = G0 @ (Jm @ E)
            assert rel_err(a[:mm].numpy(), g["coeff_cos"][k - 1]) < 1e-9 and rel_err(a[mm:].numpy(), g["coeff_sin"][k - 1]) < 1e-9
            x, v, ke, pe, per, E = ha.step(x, v, B @ a, S)
            if k in (1, 10, 50):
                assert rel_err(x.numpy(), g[f"x_{k}"]) < 1e-11 and rel_err(v.numpy(), g[f"v_{k}"]) < 1e-10, k
                assert rel_err(E.numpy(), g[f"E_mesh_{k}"]) < 1e-9, k


def test_law_action_is_g0_bit_for_bit():
    rng = np.random.default_rng(0)
    m = rng.standard_normal(10)
    m[[1, 6]] = 0.0
    m[3] = -0.0
    a = hf.law_action(hf.g0(5), m)
    want = np.concatenate([-m[:5], m[5:]])
    assert np.array_equal(a.view(np.int64), want.view(np.int64))


def _problem(seed, N=600, Ng=32, T=5, M=2):
    rng = np.random.default_rng(seed)
    S = ha.Setup(N, Ng, 50.0, 1.0, 0.1)
    x0, v0 = po.synthetic_bump_on_tail(N, S.L, seed=seed)
    G = hf.g0(M) + 0.3 * rng.standard_normal((2 * M, 2 * M))
    cot = rng.standard_normal((T, 3))
    cm = rng.standard_normal((T, 2 * M))
    cx, cv = rng.standard_normal(N), rng.standard_normal(N)
    return S, np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64), G, cot, cm, cx, cv, T, M


def test_autograd_matches_central_differences():
    S, x0, v0, G, cot, cm, cx, cv, T, M = _problem(3)
    gG, gx, gv, _, _ = hf.autograd_vjp(x0, v0, G, S, T, M, cot, cm, cx, cv)
    rng = np.random.default_rng(4)
    h = 1e-6
    for grad, base, which in ((gG, G, "G"), (gx, x0, "x"), (gv, v0, "v")):
        d = rng.standard_normal(base.shape)
        if which == "x":
            d *= 1e-2                        # (small: no particle crosses a cell edge)
        args = lambda s: dict(G=G + s * d if which == "G" else G, x0=x0 + s * d if which == "x" else x0,
                              v0=v0 + s * d if which == "v" else v0)
        f = lambda s: hf.objective(args(s)["x0"], args(s)["v0"], args(s)["G"], S, T, M, cot, cm, cx, cv)
        fd = (f(h) - f(-h)) / (2 * h)
        ad = float((grad * d).sum())
        assert abs(ad - fd) < 1e-5 * max(abs(fd), 1e-3), (which, ad, fd)


def test_hand_law_terms_match_autograd():
    """DESIGN.md 7d, section by section: m-bar_t = G^T B^T e-bar_t + cot_m_t, G-bar = sum_t a-bar_t m_t^T, E-bar_0 = J^T m-bar_0
    on the field the rollout starts from, and the x_0 part s W'(x_0) . K^T E-bar_0."""
    S, x0, v0, G, cot, cm, cx, cv, T, M = _problem(5)
    n = 2 * M
    B = torch.as_tensor(hf.basis(S.L, S.Ng, M))
    Jm = torch.as_tensor(hf.jacobian(S.Ng, M))

    def run(x0_t, E0):
        Gt = torch.as_tensor(G).clone().requires_grad_(True)
        z = torch.zeros((T, S.Ng), dtype=torch.float64, requires_grad=True)     # e-bar_t = d/dz_t
        w = torch.zeros((T, n), dtype=torch.float64, requires_grad=True)        # m-bar_t = d/dw_t
        x, v = x0_t, torch.as_tensor(v0)
        E, hist, modes = E0, [], []
        for t in range(T):
            m = Jm @ E + w[t]
            x, v, ke, pe, per, E = ha.step(x, v, B @ (Gt @ m) + z[t], S)
            hist.append(torch.stack([ke, pe, per]))
            modes.append(m)
        return hf.objective_terms(x, v, torch.stack(hist), torch.stack(modes), cot, cm, cx, cv), Gt, z, w, torch.stack(modes)

    x_leaf = torch.as_tensor(x0).clone().requires_grad_(True)
    E0 = ha.field(ha.density(torch.as_tensor(x0), S), S).detach().requires_grad_(True)
    J, Gt, z, w, modes = run(x_leaf, E0)
    gG, ez, mw, gE0, gx_open = (a.numpy() for a in torch.autograd.grad(J, (Gt, z, w, E0, x_leaf)))
    a_bar = np.stack([hf.hand_law_terms(G, ez[t], cm[t], S, M)[0] for t in range(T)])
    for t in range(T):
        _, m_bar, E_bar = hf.hand_law_terms(G, ez[t], cm[t], S, M)
        assert rel_err(m_bar, mw[t]) < 1e-10, t
        if t == 0:
            assert rel_err(E_bar, gE0) < 1e-10
    G_bar = sum(np.outer(a_bar[t], modes[t].detach().numpy()) for t in range(T))
    assert rel_err(G_bar, gG) < 1e-10
    # the field at the start read from x_0: the total x_0 gradient is the open-loop one plus the start term
    x_full = torch.as_tensor(x0).clone().requires_grad_(True)
    Jf, *_ = run(x_full, ha.field(ha.density(x_full, S), S))
    (gx_full,) = torch.autograd.grad(Jf, (x_full,))
    E_bar0 = hf.hand_law_terms(G, ez[0], cm[0], S, M)[2]
    assert rel_err(gx_open + hf.hand_start_term(x0, E_bar0, S), gx_full.numpy()) < 1e-10


def test_new_entries_are_declared_exported_and_abi_stays_5():
    from ocplasma_amd import _abi, _build
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int pic_step_feedback_gain(pic_handle* h, int max_mode, const double* gain, int mem_kind, int nsteps, "
            "double* actions_out, double* modes_out, double* hist);") in flat
    assert ("int pic_tape_backward_feedback(pic_handle* h, const double* cot_hist, const void* cot_x, const void* cot_v, "
            "const double* cot_modes, int mem_kind, double* g_ext, double* g_actions, void* g_x0, void* g_v0, "
            "double* modes_out);") in flat
    assert "ascending k" in hdr and "#define PICSTEP_ABI_VERSION 5" in hdr
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _abi.SIGNATURES["pic_step_feedback_gain"] == [vp, ci, vp, ci, ci, vp, vp, vp]
    assert _abi.SIGNATURES["pic_tape_backward_feedback"] == [vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    lib = ctypes.CDLL(_build.build_library())
    assert hasattr(lib, "pic_step_feedback_gain") and hasattr(lib, "pic_tape_backward_feedback")
    assert lib.pic_abi_version() == 5 == _abi.ABI_VERSION
