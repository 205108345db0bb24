"""Forward mode of the pooled particle features (pic_pool_jvp, pic_pool_ln_jvp) without a GPU: the exports and the
ABI, the CPU restatement (tests/hp_pool_jvp.py) against torch.func.jvp of the torch layers, against central differences of the
restated forwards and against the restated VJPs by duality, its floor against the longdouble twin, the proof that every rounded
term of an integer sum is within its stated bound (on the grid, on adversarial rows and with concentrated tangents), the work
block's layout with jvp through a stand-alone driver (also under the address and undefined-behaviour sanitizers), the compiler's
resource report of the new kernels and the Python argument checks."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import hp_pool as hp
import hp_pool_jvp as hj
import hp_pool_layout
import hp_pool_ln as hpl
from conftest import record_measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = hj.L
LAYERS = (False, True)


def _kw(p, ln):
    return dict(gamma=p[2], beta=p[3]) if ln else {}


def _case(N, H, seed, ln):
    X, V = hp.box_data(1, N, seed=seed)
    return X[0], V[0], hpl.layer(H, seed=seed + 1), hj.tangents(N, H, seed=seed + 2, ln=ln)


# ---- 1. exports and ABI -----------------------------------------------------------------------------------------------------------
def test_header_abi_and_exports_agree():
    from ocplasma_amd import _abi, _build
    hdr = " ".join(open(os.path.join(ROOT, "include", "picstep.h")).read().split())
    assert ("int pic_pool_jvp(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, int K, const void* d_x, "
            "const void* d_v, const double* d_params, int mem_kind, double* d_out);") in hdr
    assert ("int pic_pool_ln_jvp(pic_handle* h, const pic_pool_ln_spec* s, const void* x, const void* v, int K, const void* d_x, "
            "const void* d_v, const double* d_params, int mem_kind, double* d_out);") in hdr
    for text in ("dz_ik = db_k, + dW_k0 c_i, + dW_k1 s_i, + dW_k2 u_i, + (W_k1 c_i - W_k0 s_i) tq_i, + W_k2 tu_i",
                 "Z_k = |db_k|, + |dW_k0|, + |dW_k1|, + |dW_k2| u_max, + (|W_k0| + |W_k1|) tq_max, + |W_k2| tu_max",
                 "(|dgamma_k| sqrt(H) + |gamma_k| ((Z_k + (1 + sqrt(H)) Z_max) r_max)) + |dbeta_k|", "each times the margin 1 + 2^-40",
                 "for K outside 1..8"):
        assert text in hdr, text
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _abi.SIGNATURES["pic_pool_jvp"] == [vp, ctypes.POINTER(_abi.PicPoolSpec), vp, vp, ci, vp, vp, vp, ci, vp]
    assert _abi.SIGNATURES["pic_pool_ln_jvp"] == [vp, ctypes.POINTER(_abi.PicPoolLnSpec), vp, vp, ci, vp, vp, vp, ci, vp]
    assert callable(_abi.Handle.pool_jvp) and callable(_abi.Handle.pool_ln_jvp)
    lib = ctypes.CDLL(_build.build_library())
    assert lib.pic_pool_jvp and lib.pic_pool_ln_jvp
    assert lib.pic_abi_version() == 5 and _abi.ABI_VERSION == 5 and "#define PICSTEP_ABI_VERSION 5" in hdr


# ---- 2. the restatement three ways --------------------------------------------------------------------------------------------------
def _torch_layer(x, v, W, b, gamma, beta, act, ln):
    q = 2 * np.pi * x / L
    n = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1) @ W.T + b
    if ln:
        n = torch.nn.functional.layer_norm(n, (len(b),), gamma, beta, 1e-5)
    return (torch.tanh(n) if act == "tanh" else torch.relu(n)).mean(dim=0)


@pytest.mark.parametrize("ln", LAYERS)
@pytest.mark.parametrize("N", [1, 63, 1025])
def test_restatement_matches_torch_func_jvp(N, ln):
    """Against torch.func.jvp of the float64 torch layers (layer_norm included), relative to each output's contract bound.  torch's
    float64 is as far from the twin as the restatement is: twice the device's bound."""
    worst = 0.0
    for H, act in itertools.product((2, 5, 64), hj.ACTS):
        x, v, p, t = _case(N, H, seed=100 * H + N, ln=ln)
        prim = tuple(torch.tensor(a) for a in (x, v, *p))
        tang = tuple(torch.tensor(t[k]) if k in t else torch.zeros_like(a) for k, a in zip(hj.NAMES, prim))
        ref = torch.func.jvp(lambda *a: _torch_layer(*a, act, ln), prim, tang)[1].numpy()
        mine = hj.jvp(x, v, p[0], p[1], L, act, **_kw(p, ln), **t)
        worst = max(worst, hj.rel_error(mine, ref, hj.term_bounds(x, v, p[0], p[1], L, act, **_kw(p, ln), **t)))
    record_measure(f"pool_jvp_restatement_vs_torch_{'ln' if ln else 'plain'}_N{N}", worst)
    assert worst < 2 * hj.bound(ln, N), worst


@pytest.mark.parametrize("ln", LAYERS)
@pytest.mark.parametrize("activation,tol", [("tanh", 1e-7), ("relu", 1e-4)])
def test_restatement_matches_central_differences_of_the_restated_forward(activation, tol, ln):
    """h = 1e-6 and the bounds of tests/test_pool_ln_cpu.py's check of the hand VJP: the differences of two float64 results give
    1e-9, and for relu the particles within h of a kink carry the wrong slope: 1e-6.  100 x each."""
    N, H, h = 501, 5, 1e-6
    errs = []
    for seed in range(3):
        x, v, p, t = _case(N, H, seed=11 + seed, ln=ln)
        cot = np.random.default_rng(seed).normal(0.0, 1.0, H)
        args = [x, v, *(p if ln else p[:2])]
        d = [t[k] for k in hj.NAMES[:len(args)]]
        fwd = (lambda *a: hpl.forward(*a, L, activation)) if ln else (lambda *a: hp.forward(*a, L, activation))
        f = lambda sgn: float(np.dot(cot, fwd(*(a + sgn * h * di for a, di in zip(args, d)))))      # noqa: E731
        lin = float(np.dot(cot, hj.jvp(x, v, p[0], p[1], L, activation, **_kw(p, ln), **t)))
        errs.append(abs(lin - (f(1.0) - f(-1.0)) / (2.0 * h)) / abs(lin))
    record_measure(f"pool_jvp_restatement_fd_{'ln' if ln else 'plain'}_{activation}", max(errs))
    assert max(errs) < tol, errs


def test_restatement_is_dual_to_the_restated_vjps():
    """<cot, jvp> = <vjp, tangent> between the float64 restatements, relative to sum_k |cot_k| B_k: both are within their floors
    (a few 1e-16 to 1e-15 of that scale, tests/hp_pool*.py) of the exact value, so the gap is below 100 x their sum."""
    worst = 0.0
    for (N, H), ln, act in itertools.product(((1, 1), (63, 5), (1025, 5), (4097, 64)), LAYERS, hj.ACTS):
        x, v, p, t = _case(N, H, seed=N + H, ln=ln)
        cot = np.random.default_rng(N).normal(0.0, 1.0, H)
        worst = max(worst, hj.duality_gap(x, v, p[0], p[1], cot, L, act, **_kw(p, ln), **t))
    record_measure("pool_jvp_restatement_duality", worst)
    fl = hj.floor()
    assert worst < 100.0 * (fl["plain"] + fl["ln"] + hpl.floor()["vjp"] + hp.floor()["vjp"]), worst


def test_restatement_is_order_free_direction_free_and_scales_by_powers_of_two():
    x, v, p, t = _case(1025, 5, seed=3, ln=True)
    perm = np.random.default_rng(0).permutation(1025)
    for ln, act in itertools.product(LAYERS, hj.ACTS):
        tt = {k: a for k, a in t.items() if ln or k not in ("d_gamma", "d_beta")}
        out = hj.jvp(x, v, p[0], p[1], L, act, **_kw(p, ln), **tt)
        tp = dict(tt, d_x=tt["d_x"][perm], d_v=tt["d_v"][perm])
        assert np.array_equal(out, hj.jvp(x[perm], v[perm], p[0], p[1], L, act, **_kw(p, ln), **tp))
        for scale in (2.0 ** 300, 2.0 ** -300, 0.0):
            ts = {k: a * scale for k, a in tt.items()}
            assert np.array_equal(out * scale, hj.jvp(x, v, p[0], p[1], L, act, **_kw(p, ln), **ts)), scale
    # H = 1 with the LayerNorm: every dy is +0, the term is exactly a dbeta
    p1, t1 = hpl.layer(1, seed=5), hj.tangents(1025, 1, seed=6, ln=True)
    audit = {}
    out = hj.jvp(x, v, p1[0], p1[1], L, "relu", gamma=p1[2], beta=p1[3], audit=audit, **t1)
    assert audit["dy"] == 0.0
    B = hj.term_bounds(x, v, p1[0], p1[1], L, "relu", gamma=p1[2], beta=p1[3], **t1)
    assert abs(out[0] - (t1["d_beta"][0] if p1[3][0] > 0 else 0.0)) <= 2.0 * 1025 * 2.0 ** -61 * B[0]


# ---- 3. the floor -----------------------------------------------------------------------------------------------------------------
def test_floor_against_the_longdouble_twin():
    fl = hj.floor()
    record_measure("pool_jvp_floor_plain", fl["plain"])
    record_measure("pool_jvp_floor_ln", fl["ln"])
    # float64 rounding of a depth of a few H plus the unit's resolution at N = 8193 (7e-15): far above means the two have parted
    assert 0 < fl["plain"] < 1e-13 and 0 < fl["ln"] < 1e-13, fl
    # the floor's grid: every term inside its bound, no relu argument nearer to the kink than 7s allows
    assert fl["audit"]["d_out"] <= 1.0 and fl["audit"]["n_min"] >= hpl.N_MIN, fl["audit"]


# ---- 4. every rounded term is within its stated bound -------------------------------------------------------------------------------
def test_terms_are_within_their_bounds_on_the_device_tests_grid():
    worst, n_min = 0.0, np.inf
    for N, H in itertools.product(hj.GRID_N, hj.GRID_H):
        if N * H > 64 * 1025 and (N, H) != (4097, 256):
            continue                                        # (the large shapes cost seconds each and add one more of the same)
        X, V, sets, _ = hpl.grid_case(N, H)
        dX, dV, tsets = hj.grid_tangents(N, H)
        for ln, act in itertools.product(LAYERS, hj.ACTS):
            audit = {}
            hj.jvp(X[0], V[0], sets[0][0], sets[0][1], L, act, **_kw(sets[0], ln), audit=audit, d_x=dX[0][0], d_v=dV[0][0],
                   **{k: tsets[0][k][0] for k in hj.PARAM_T[ln]})
            worst = max(worst, audit.get("d_out", 0.0))
            if act == "relu" and not (ln and H == 1):
                n_min = min(n_min, audit["n_min"])
    record_measure("pool_jvp_grid_term_over_bound", worst)
    record_measure("pool_jvp_grid_relu_n_min", n_min)
    assert worst <= 1.0 and n_min >= hpl.N_MIN, (worst, n_min)


@pytest.mark.parametrize("eps", [1e-5, 1e-12, 1.0])
def test_terms_are_within_their_bounds_on_adversarial_rows_and_concentrated_tangents(eps):
    """7s's adversarial rows (equal rows, one dominating unit, a mean that rounds) under random tangents and under tangents
    concentrated on one particle or on one unit."""
    N = 257
    X, V = hp.box_data(1, N, seed=7)
    worst = 0.0
    for H in (2, 16, 64):
        W, b, gamma, beta = hpl.layer(H, seed=5)
        rows = {"plain": (W, b), "equal": (np.broadcast_to(W[0], (H, 3)).copy(), np.full(H, b[0]))}
        Wd, bd = 1e-9 * W, 1e-9 * b
        Wd[H // 2], bd[H // 2] = (3.0, -2.0, 5.0), 1e6
        rows["dominant"] = (Wd, bd)
        bh = np.full(H, 2.0 ** 53)
        bh[1] += 2.0
        rows["rounded mean"] = (np.zeros((H, 3)), bh)
        full = hj.tangents(N, H, seed=8, ln=True)
        one_particle = {k: np.zeros_like(a) for k, a in full.items()}
        one_particle["d_x"][N // 2], one_particle["d_v"][N // 3] = 1e3, -1e3
        one_unit = {k: np.zeros_like(a) for k, a in full.items()}
        one_unit["d_W"][H // 2], one_unit["d_b"][H // 2], one_unit["d_gamma"][H // 2] = (1e3, -1e3, 1e3), 1e3, 1.0
        skew = dict(full, d_W=full["d_W"] * 1e-6, d_x=full["d_x"] * 1e6)
        for (name, (Wa, ba)), t, ln, act in itertools.product(rows.items(), (full, one_particle, one_unit, skew), LAYERS, hj.ACTS):
            audit = {}
            tt = {k: a for k, a in t.items() if ln or k not in ("d_gamma", "d_beta")}
            hj.jvp(X[0], V[0], Wa, ba, L, act, **(dict(gamma=gamma, beta=beta, eps=eps) if ln else {}), audit=audit, **tt)
            assert audit.get("d_out", 0.0) <= 1.0, (name, H, ln, act, eps, audit)
            worst = max(worst, audit.get("d_out", 0.0))
    record_measure(f"pool_jvp_adversarial_term_over_bound_eps{eps:g}", worst)


# ---- 5. the work block's layout with jvp --------------------------------------------------------------------------------------------
FLAGS, TFLAGS = "per_env host params_host xv".split(), "d_x d_v d_params".split()


def _bits(names, **kw):
    assert set(kw) <= set(names)
    return sum(1 << i for i, f in enumerate(names) if kw.get(f))


def _build_driver(tmp, name, extra):
    import shutil
    import subprocess
    out = str(tmp / name)
    args = ["-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + hp_pool_layout.CSRC] + extra + \
           [os.path.join(ROOT, "tests", "pool_jvp_driver.cpp"), "-o", out]
    cxx = shutil.which("c++")
    if cxx:
        cmd = [cxx] + args
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no host C++ compiler (c++ or hipcc) to build tests/pool_jvp_driver.cpp with")
        cmd = [hipcc, "-x", "c++"] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        res = p.stdout.splitlines()
        assert len(res) == len(lines)
        return res
    return run


def _model(ln, E, N, H, f, K, tf):
    """The layout restated: the parts in order, each rounded up to 256 bytes; a part without elements has no view; the tangents'
    max words lie inside the first part, behind the environment's own (two with the LayerNorm)."""
    on = {k: bool(f >> i & 1) for i, k in enumerate(FLAGS)}
    on.update({k: bool(tf >> i & 1) for i, k in enumerate(TFLAGS)})
    P, rows, own = (6 if ln else 4) * H, E * N, (2 if ln else 1) * E
    vecs = E if on["per_env"] else 1
    parts = [("max", own + 2 * K * E), ("acc", K * E * H), ("gE", 0), ("params", vecs * P if on["params_host"] else 0),
             ("d_params", K * vecs * P if on["d_params"] and on["params_host"] else 0)]
    host = [("x", rows if on["xv"] else 0), ("v", rows if on["xv"] else 0), ("cot", 0), ("out", K * E * H), ("g_x", 0), ("g_v", 0), ("g", 0),
            ("d_x", K * rows if on["d_x"] else 0), ("d_v", K * rows if on["d_v"] else 0)]
    parts += host if on["host"] else [(k, 0) for k, _ in host]
    at, views, spans = 0, {}, []
    for name, count in parts:
        views[name] = f"{name}={at if count else 'null'}"
        if count:
            spans.append((at, at + 8 * count))
        at = (at + 8 * count + 255) // 256 * 256
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= at
    views["tmax"] = f"tmax={8 * own}"
    order = "max tmax acc gE params d_params x v cot out g_x g_v g d_x d_v".split()
    return f"ok pool={at} " + " ".join(views[k] for k in order)


TABLE = [
    # a device call of the stored particles, K = 3: 2 + 12 max words, 3 x 2 x 32 sums
    (False, f"2 1000 32 {_bits(FLAGS)} 3 {_bits(TFLAGS, d_x=1)}",
     "ok pool=1792 max=0 tmax=16 acc=256 gE=null params=null d_params=null x=null v=null cot=null out=null g_x=null g_v=null g=null "
     "d_x=null d_v=null"),
    # the LayerNorm: r_max behind u_max, the tangents' words behind both
    (True, f"2 1000 32 {_bits(FLAGS)} 3 {_bits(TFLAGS, d_x=1)}",
     "ok pool=1792 max=0 tmax=32 acc=256 gE=null params=null d_params=null x=null v=null cot=null out=null g_x=null g_v=null g=null "
     "d_x=null d_v=null"),
    # a host call that gives everything, K = 8, one environment, one particle, one unit
    (False, f"1 1 1 {_bits(FLAGS, host=1, params_host=1, xv=1)} 8 {_bits(TFLAGS, d_x=1, d_v=1, d_params=1)}",
     "ok pool=2304 max=0 tmax=8 acc=256 gE=null params=512 d_params=768 x=1024 v=1280 cot=null out=1536 g_x=null g_v=null g=null "
     "d_x=1792 d_v=2048"),
]


def test_pool_parts_with_jvp_table_and_model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pool_jvp")
    runs = (_build_driver(tmp, "pool_jvp_driver", []),
            _build_driver(tmp, "pool_jvp_driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))
    for ln, cfg, want in TABLE:
        assert want == _model(ln, *map(int, cfg.split())), cfg          # (the table pins the model, the model the sweep)
    cases = [(ln, f"{E} {N} {H} {f} {K} {tf}") for ln, E, N, H, f, K, tf in
             itertools.product(LAYERS, (1, 3, 17, 300), (1, 4097), (1, 33, 256), range(16), (1, 3, 8), range(8))]
    cases = [(ln, cfg) for ln, cfg, _ in TABLE] + cases
    for run in runs:
        got = run([("ln " if ln else "") + cfg for ln, cfg in cases])
        for (ln, cfg), g in zip(cases, got):
            assert g == _model(ln, *map(int, cfg.split())), (ln, cfg)


# ---- 6. the compiler's resource report -----------------------------------------------------------------------------------------------
def test_new_kernels_have_no_scratch():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    for name in ("pool_jvp_max_kernel", "pool_jvp_kernel", "pool_jvp_finish_kernel", "pool_ln_jvp_max_kernel", "pool_ln_jvp_kernel",
                 "pool_ln_jvp_finish_kernel"):
        hits = [v for k, v in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1, name
        assert hits[0]["scratch_bytes_per_lane"] == 0 and hits[0]["lds_bytes_per_block"] <= 16 * 1024, (name, hits[0])
    # the max kernels of the forward and the VJP are still there, as they were
    for name in ("pool_max_kernel", "pool_ln_max_kernel"):
        hits = [v for k, v in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1 and hits[0]["scratch_bytes_per_lane"] == 0, name


# ---- 7. the Python argument checks need no device ------------------------------------------------------------------------------------
def _bare_env(E=2, N=10):
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC.__new__(BatchedPIC)            # no handle: a check that reached the library would raise AttributeError
    env.num_envs, env.N = E, N
    return env


@pytest.mark.parametrize("kw,msg", [
    (dict(d_x=np.zeros((2, 9))), r"pool_jvp: d_x must have shape \(2, 10\)"),
    (dict(d_v=np.zeros((3, 2, 9))), r"pool_jvp: d_v must have shape \(3, 2, 10\)"),
    (dict(d_x=np.zeros((3, 2, 10)), d_v=np.zeros((2, 2, 10))), "pool_jvp: the inputs disagree on the number of directions"),
    (dict(d_x=np.zeros((3, 2, 10)), d_b=np.zeros(4)), r"pool_jvp: d_b must have shape \(3, 4\)"),
    (dict(d_W=np.zeros((4, 2))), r"pool_jvp: d_W must have shape \(4, 3\)"),
    (dict(d_gamma=np.zeros(4)), "pool_jvp: d_gamma and d_beta need gamma and beta"),
    (dict(gamma=np.ones(4), beta=np.zeros(4), d_beta=np.zeros(5)), r"pool_jvp: d_beta must have shape \(4,\)"),
    (dict(gamma=np.ones(4)), "pool_jvp: gamma and beta must both be given"),
    (dict(W=np.zeros((257, 3)), b=np.zeros(257)), "pool_jvp: H must be 1..256"),
    (dict(x=np.zeros((2, 10))), "pool_jvp: x and v must both be given"),
    (dict(activation="gelu"), "pool_jvp: activation must be one of"),
    (dict(v_scale=float("inf")), "pool_jvp: v_scale must be finite"),
    (dict(gamma=np.ones(4), beta=np.zeros(4), eps=0.0), "pool_jvp: eps must be finite and > 0"),
])
def test_argument_checks_raise_before_the_device(kw, msg):
    args = dict(W=np.zeros((4, 3)), b=np.zeros(4))
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        _bare_env().pool_jvp(**args)
