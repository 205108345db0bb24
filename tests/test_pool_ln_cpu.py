"""The pooled particle features with a LayerNorm (pic_pool_ln, pic_pool_ln_vjp) without a GPU: the exports and the
ABI, the CPU restatement (tests/hp_pool_ln.py) against the reference encoder's recorded results (tests/golden/g19), against
torch.nn.LayerNorm + autograd over the device test's grid and against central differences, its floor against the longdouble
twin, the proof that every term of an integer sum is within its stated bound (on the grid and on adversarial rows), the distance
of every relu pre-activation from the kink, the work block's layout through a stand-alone driver (also under the address and
undefined-behaviour sanitizers), the compiler's resource report of the new kernels and the Python argument checks."""
import ctypes
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import hp_pool as hp
import hp_pool_layout
import hp_pool_ln as hpl
from conftest import record_measure
from hp_pool_layout import _flags, drivers  # noqa: F401  (drivers: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = hpl.L
G19, PHI = hpl.G19, hpl.PHI


# ---- 1. exports and ABI -----------------------------------------------------------------------------------------------------------
def test_header_abi_and_exports_agree():
    from ocplasma_amd import _abi, _build
    hdr = " ".join(open(os.path.join(ROOT, "include", "picstep.h")).read().split())
    assert ("typedef struct pic_pool_ln_spec { int32_t hidden, activation, per_env, params_mem_kind; double v_scale, eps, period; "
            "const double* params; } pic_pool_ln_spec;") in hdr
    assert "int pic_pool_ln(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, int mem_kind, double* out);" in hdr
    assert ("int pic_pool_ln_vjp(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, const double* cot, "
            "int mem_kind, void* g_x, void* g_v, double* g_params);") in hdr
    assert [n for n, _ in _abi.PicPoolLnSpec._fields_] == ["hidden", "activation", "per_env", "params_mem_kind", "v_scale", "eps",
                                                           "period", "params"]
    assert ctypes.sizeof(_abi.PicPoolLnSpec) == 4 * 4 + 3 * 8 + 8
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _abi.SIGNATURES["pic_pool_ln"] == [vp, ctypes.POINTER(_abi.PicPoolLnSpec), vp, vp, ci, vp]
    assert _abi.SIGNATURES["pic_pool_ln_vjp"] == [vp, ctypes.POINTER(_abi.PicPoolLnSpec), vp, vp, vp, ci, vp, vp, vp]
    lib = ctypes.CDLL(_build.build_library())
    assert lib.pic_pool_ln and lib.pic_pool_ln_vjp
    assert lib.pic_abi_version() == 5 and _abi.ABI_VERSION == 5 and "#define PICSTEP_ABI_VERSION 5" in hdr


# ---- 2. the restatement against the reference encoder (g19) -------------------------------------------------------------------------
_g19, g19_restated = hpl.g19_case, hpl.g19_restated


def test_restatement_matches_the_reference_encoder():
    ef, eg = hpl.g19_restatement_error()
    record_measure("pool_ln_restatement_vs_g19_forward", ef)
    record_measure("pool_ln_restatement_vs_g19_vjp", eg)
    # the issue's own CPU check of these formulas found 1.6e-15 (forward) and 5e-14 (parameter sums, absolute); relative to the
    # contract bounds that is less.  torch's float64 is as far from the twin as the restatement is: twice the bound.
    assert ef < 2 * hpl.bound("forward", 513) and eg < 2 * hpl.bound("vjp", 513), (ef, eg)


def test_restatement_through_rho_matches_the_reference_encoder():
    """The encoder's output and the gradients of <cot_enc, enc> with respect to x, v and all eight tensors: the restatement's
    phi and mean, rho as float64 torch layers, the chain rule through the hand VJP."""
    for pre in hpl.G19_CASES:
        g, sd, period, v_scale = _g19(pre)
        p = [sd[k] for k in PHI]
        out, _ = g19_restated(pre)
        lin = torch.nn.Linear(int(g["H"]), int(g["H_out"]), dtype=torch.float64)
        norm = torch.nn.LayerNorm(int(g["H_out"]), dtype=torch.float64)
        with torch.no_grad():
            for t, k in ((lin.weight, "rho.0.weight"), (lin.bias, "rho.0.bias"), (norm.weight, "rho.1.weight"), (norm.bias, "rho.1.bias")):
                t.copy_(torch.as_tensor(sd[k]))
        pooled = torch.tensor(out, requires_grad=True)
        enc = torch.relu(norm(lin(pooled)))
        assert np.max(np.abs(enc.detach().numpy() - g["enc"])) < 1e-12, pre
        gr = torch.autograd.grad((enc * torch.as_tensor(g["cot_enc"])).sum(), [pooled, lin.weight, lin.bias, norm.weight, norm.bias])
        for got, k in zip(gr[1:], ("rho.0.weight", "rho.0.bias", "rho.1.weight", "rho.1.bias")):
            assert np.max(np.abs(got.numpy() - g["genc_" + k])) < 1e-12, (pre, k)
        cot = gr[0].numpy()
        grads = [hpl.vjp(g["x"][e], g["v"][e], *p, cot[e], period, "relu", v_scale) for e in range(len(out))]
        for e in range(len(out)):
            assert np.max(np.abs(grads[e][0] - g["genc_x"][e])) < 1e-12 and np.max(np.abs(grads[e][1] - g["genc_v"][e])) < 1e-12, pre
        for i, k in enumerate(PHI):
            assert np.max(np.abs(sum(gr_[2 + i] for gr_ in grads) - g["genc_" + k])) < 1e-11, (pre, k)


def test_one_hidden_unit_gives_exact_zeros():
    """H = 1 (g19's case c): d = 0, y = 0, out = relu(beta), every dz exactly +0 -- where autograd returns roundoff / sqrt(eps)."""
    g, sd, period, v_scale = _g19("c")
    out, grads = g19_restated("c")
    assert np.array_equal(out, np.broadcast_to(np.maximum(sd["phi.1.bias"], 0.0), out.shape))
    for gr in grads:
        for a in gr[:4]:
            assert np.array_equal(a, np.zeros_like(a)) and not np.signbit(a).any()


# ---- 3. the restatement against torch.nn.LayerNorm + autograd over the device test's grid ------------------------------------------
def _torch_layer(x, v, W, b, gamma, beta, act):
    q = 2 * np.pi * x / L
    f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1)
    n = torch.nn.functional.layer_norm(f @ W.T + b, (len(b),), gamma, beta, 1e-5)
    return (torch.tanh(n) if act == "tanh" else torch.relu(n)).mean(dim=0)


@pytest.mark.parametrize("N", hpl.GRID_N)
def test_restatement_matches_torch_layernorm_over_the_grid(N):
    worst = [0.0, 0.0]
    for H in hpl.GRID_H:
        X, V, sets, cot = hpl.grid_case(N, H)
        for act in hpl.ACTS:
            mine = hpl.restated(N, H, 0, 0, act)[0]
            t = [torch.tensor(a, requires_grad=True) for a in (X[0], V[0], *sets[0])]
            out = _torch_layer(*t, act)
            gr = torch.autograd.grad((out * torch.tensor(cot[0])).sum(), t)
            ref = (out.detach().numpy(),) + tuple(a.numpy() for a in gr)
            if H == 1:                  # autograd's g_x, g_v, g_W, g_b are roundoff / sqrt(eps) here; the contract's are exact zeros
                assert all(np.array_equal(a, np.zeros_like(a)) for a in mine[1:5])
            ef, eg = hpl.errors(mine[0], mine[1:], ref, X[0], V[0], *sets[0], cot[0], L, act)
            worst = [max(worst[0], ef), max(worst[1], eg)]
    record_measure(f"pool_ln_restatement_vs_torch_forward_N{N}", worst[0])
    record_measure(f"pool_ln_restatement_vs_torch_vjp_N{N}", worst[1])
    assert worst[0] < 2 * hpl.bound("forward", N) and worst[1] < 2 * hpl.bound("vjp", N), worst


# ---- 4. the floor -----------------------------------------------------------------------------------------------------------------
def test_floor_against_the_longdouble_twin():
    fl = hpl.floor()
    record_measure("pool_ln_floor_forward", fl["forward"])
    record_measure("pool_ln_floor_vjp", fl["vjp"])
    # float64 rounding of a depth of a few H plus the unit's resolution at N = 4097 (4e-15): far above means the two have parted
    assert 0 < fl["forward"] < 1e-13 and 0 < fl["vjp"] < 1e-13, fl


# ---- 5. every term of an integer sum is within its stated bound ----------------------------------------------------------------------
GRID_RUNS = [(0, 0), (1, 0), (2, 0), (0, 1)]          # (environment, parameter set) of the device's parity test


def _assert_audit(audit, where):
    # |y| / sqrt(H) <= 1 up to the four roundings of var + eps, sqrt, 1 / and d r (half an ulp each) and sqrt(H)'s own: 2^-51; the
    # bounds' margins (1 + 2^-50, 1 + 2^-40) are above that, so the terms themselves never exceed their bounds
    assert audit.get("y", 0.0) <= 1.0 + 2.0 ** -51, (where, "y", audit["y"])
    for key in ("out", "g_W", "g_b", "g_gamma", "g_beta"):
        assert audit.get(key, 0.0) <= 1.0, (where, key, audit[key])


def test_terms_are_within_their_bounds_and_relu_is_off_the_kink_on_the_grid():
    n_min = np.inf
    for N, H in itertools.product(hpl.GRID_N, hpl.GRID_H):
        for e, s in GRID_RUNS:
            for act in hpl.ACTS if (e, s) == (0, 0) else ("relu",):
                audit = hpl.restated(N, H, e, s, act)[1]
                _assert_audit(audit, (N, H, e, s, act))
                if act == "relu" and H > 1:          # (H = 1: n = beta exactly, on the device too)
                    n_min = min(n_min, audit["n_min"])
    record_measure("pool_ln_grid_relu_n_min", n_min)
    assert n_min >= hpl.N_MIN, n_min


@pytest.mark.parametrize("eps", [1e-5, 1e-12, 1.0])
def test_terms_are_within_their_bounds_on_adversarial_rows(eps):
    N = 257
    X, V = hp.box_data(1, N, seed=7)
    worst = {}
    for H in (2, 16, 64):
        W, b, gamma, beta = hpl.layer(H, seed=5)
        cot = np.random.default_rng(6).normal(0.0, 1.0, H)
        rows = {}
        We = np.broadcast_to(W[0], (H, 3)).copy()                        # all rows of W equal (and b): var = 0, r = 1 / sqrt(eps)
        rows["equal"] = (We, np.full(H, b[0]))
        Wd, bd = 1e-9 * W, 1e-9 * b                                      # one unit dominating: |y| -> sqrt(H - 1)
        Wd[H // 2], bd[H // 2] = (3.0, -2.0, 5.0), 1e6
        rows["dominant"] = (Wd, bd)
        Wh = np.zeros((H, 3))                                            # a mean that rounds: z = (2^53, 2^53 + 2, 2^53, ...)
        bh = np.full(H, 2.0 ** 53)
        bh[1] += 2.0
        rows["rounded mean"] = (Wh, bh)
        for name, (Wa, ba) in rows.items():
            for act in hpl.ACTS:
                audit = {}
                hpl.forward(X[0], V[0], Wa, ba, gamma, beta, L, act, eps=eps, audit=audit)
                hpl.vjp(X[0], V[0], Wa, ba, gamma, beta, cot, L, act, eps=eps, audit=audit)
                _assert_audit(audit, (name, H, act, eps))
                for k, val in audit.items():
                    if k != "n_min":
                        worst[k] = max(worst.get(k, 0.0), val)
        # the rows do what they are there for
        q, u = hp.features(X[0], V[0], L, 1.0)
        assert np.all(hpl.stats(np.cos(q), np.sin(q), u, *rows["equal"], eps)[1] == 1.0 / np.sqrt(eps))
    assert worst["y"] > 0.98, worst                                     # (|y| = sqrt(63) at H = 64: 0.992 sqrt(H))
    for k, val in worst.items():
        record_measure(f"pool_ln_adversarial_{k}_eps{eps:g}", val)


# ---- 6. the hand VJP against central differences -----------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,tol", [("tanh", 1e-7), ("relu", 1e-4)])
def test_hand_vjp_matches_central_differences(activation, tol):
    """eps = 1e-6 as for the plain layer (tests/test_pool_cpu.py): the differences of two float64 results give 1e-9, and for relu
    the particles within eps of a kink carry the wrong slope: 1e-6.  100 x each."""
    N, H, h = 501, 5, 1e-6
    x, v, _, _, cot = hp.case(N, H, seed=11)
    args = [x, v, *hpl.layer(H, seed=4)]
    errs = []
    for seed in range(3):
        d = [np.random.default_rng(seed).standard_normal(a.shape) for a in args]
        g = hpl.vjp(*args, cot, L, activation)
        lin = sum(float(np.sum(gi * di)) for gi, di in zip(g, d))
        f = lambda sgn: float(np.dot(cot, hpl.forward(*(a + sgn * h * di for a, di in zip(args, d)), L, activation)))
        errs.append(abs(lin - (f(1.0) - f(-1.0)) / (2.0 * h)) / abs(lin))
    record_measure(f"pool_ln_restatement_fd_{activation}", max(errs))
    assert max(errs) < tol, errs


def test_restatement_is_order_free_and_scales_by_powers_of_two():
    X, V, sets, cot = hpl.grid_case(1025, 5)
    perm = np.random.default_rng(0).permutation(1025)
    for act in hpl.ACTS:
        out, g = hpl.forward(X[0], V[0], *sets[0], L, act), hpl.vjp(X[0], V[0], *sets[0], cot[0], L, act)
        assert np.array_equal(out, hpl.forward(X[0][perm], V[0][perm], *sets[0], L, act))
        gp = hpl.vjp(X[0][perm], V[0][perm], *sets[0], cot[0], L, act)
        assert np.array_equal(g[0][perm], gp[0]) and all(np.array_equal(a, c) for a, c in zip(g[2:], gp[2:]))
        for scale in (2.0 ** 100, 2.0 ** -100):
            gs = hpl.vjp(X[0], V[0], *sets[0], cot[0] * scale, L, act)
            assert all(np.array_equal(a * scale, c) for a, c in zip(g, gs)), scale


# ---- 7. the work block's layout ---------------------------------------------------------------------------------------------------
LN = True                       # (hp_pool_layout: the drivers fixture)
_model = functools.partial(hp_pool_layout._model, ln=LN)

TABLE = [
    # a device forward of the stored particles: the max words and H sums per environment, nothing else
    (f"2 1000 32 {_flags()}", "ok pool=768 max=0 acc=256 gE=null params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # a device VJP with shared parameters: two max words per environment, 6H sums, the rows the reduction reads
    (f"2 1000 32 {_flags(vjp=1, g_x=1, g_v=1, g_params=1)}",
     "ok pool=6400 max=0 acc=256 gE=3328 params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # ... with per-environment parameters the sums go straight to the caller
    (f"2 1000 32 {_flags(vjp=1, per_env=1, g_params=1)}",
     "ok pool=3328 max=0 acc=256 gE=null params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # 17 environments: the VJP's 34 max words need a second 256 bytes
    (f"17 10 1 {_flags(vjp=1)}", "ok pool=1536 max=0 acc=512 gE=null params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # a host VJP that gives and wants everything: E N 8 = 16000 bytes round up to 16128
    (f"2 1000 32 {_flags(vjp=1, host=1, params_host=1, xv=1, g_x=1, g_v=1, g_params=1)}",
     "ok pool=74496 max=0 acc=256 gE=3328 params=6400 x=7936 v=24064 cot=40192 out=null g_x=40704 g_v=56832 g=72960"),
    # a host forward with one environment, one particle, one unit
    (f"1 1 1 {_flags(host=1, params_host=1, xv=1)}",
     "ok pool=1536 max=0 acc=256 gE=null params=512 x=768 v=1024 cot=null out=1280 g_x=null g_v=null g=null"),
]


def test_pool_ln_parts_table_and_model(drivers):
    plain, sanitized = drivers
    for cfg, want in TABLE:
        E, N, H, f = map(int, cfg.split())
        assert want == _model(E, N, H, f), cfg              # (the table pins the model, the model the sweep)
    lines = [f"{E} {N} {H} {f}" for E, N, H, f in itertools.product((1, 3, 17, 300), (1, 63, 4097), (1, 5, 33, 256), range(256))]
    lines = [cfg for cfg, _ in TABLE] + lines
    for run in (plain, sanitized):
        got = run(lines)
        for cfg, g in zip(lines, got):
            E, N, H, f = map(int, cfg.split())
            assert g == _model(E, N, H, f), cfg


# ---- 8. the compiler's resource report -----------------------------------------------------------------------------------------------
def test_new_kernels_have_no_scratch():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    for name in ("pool_ln_kernel", "pool_ln_finish_kernel", "pool_ln_max_kernel", "pool_ln_vjp_kernel", "pool_ln_vjp_finish_kernel"):
        hits = [v for k, v in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, name
        assert hits[0]["scratch_bytes_per_lane"] == 0 and hits[0]["agprs"] == 0, (name, hits[0])
        assert hits[0]["vgprs"] <= 256 and hits[0]["lds_bytes_per_block"] <= 16 * 1024, (name, hits[0])
    # the plain layer's kernels are still there, as they were: zero scratch
    for name in ("pool_kernel", "pool_vjp_kernel", "pool_max_kernel", "pool_finish_kernel", "pool_vjp_finish_kernel"):
        hits = [v for k, v in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1 and hits[0]["scratch_bytes_per_lane"] == 0, name


# ---- 9. the Python argument checks need no device ------------------------------------------------------------------------------------
def _bare_env(E=2, N=10):
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC.__new__(BatchedPIC)            # no handle: a check that reached the library would raise AttributeError
    env.num_envs, env.N = E, N
    return env


@pytest.mark.parametrize("kw,msg", [
    (dict(beta=None), "gamma and beta must both be given"),
    (dict(gamma=None), "gamma and beta must both be given"),
    (dict(gamma=np.ones(5)), "gamma must have shape"),
    (dict(beta=np.ones((2, 4))), "beta must have shape"),
    (dict(eps=0.0), "eps must be finite and > 0"),
    (dict(eps=-1e-5), "eps must be finite and > 0"),
    (dict(eps=float("nan")), "eps must be finite and > 0"),
    (dict(eps=float("inf")), "eps must be finite and > 0"),
    (dict(period=-1.0), "period must be finite and >= 0"),
    (dict(period=float("inf")), "period must be finite and >= 0"),
    (dict(W=np.zeros((257, 3)), b=np.zeros(257), gamma=np.ones(257), beta=np.zeros(257)), "H must be 1..256"),
    (dict(x=np.zeros((2, 10))), "both be given"),
])
def test_argument_checks_raise_before_the_device(kw, msg):
    env = _bare_env()
    args = dict(W=np.zeros((4, 3)), b=np.zeros(4), gamma=np.ones(4), beta=np.zeros(4))
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        env.pool(**args)
    with pytest.raises(ValueError, match=msg):
        env.pool_vjp(cot=np.zeros((2, np.shape(args["b"])[-1])), **args)
