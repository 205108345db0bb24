"""The pooled particle features (pic_pool, pic_pool_vjp) without a GPU: the CPU restatement (tests/hp_pool.py)
against torch and against finite differences, its floor against the longdouble twin, the work block's layout and the passes'
launch plan through a stand-alone driver (also under the address and undefined-behaviour sanitizers), the Python argument checks,
and the preconditions of the device's edge tests (tests/test_gpu_pool_edges.py) on the restatement."""
import os

import numpy as np
import pytest
import torch

import hp_policy as hpp
import hp_pool as hp
from conftest import record_measure
from hp_pool_layout import _flags, _model, drivers  # noqa: F401  (drivers: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 50.0


# ---- 1. the restatement against torch ---------------------------------------------------------------------------------------------
def _torch_phi_mean(x, v, W, b):
    """hp_policy.deepsets_state's phi and mean (its rho left out): h.mean over the particles, float64 torch."""
    q = 2 * np.pi * x / L
    f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1)
    return torch.tanh(torch.einsum("...nk,...hk->...nh", f, W) + b.unsqueeze(-2)).mean(dim=-2)


@pytest.mark.parametrize("N,H", [(63, 5), (5000, 64)])
def test_restatement_matches_torch_and_autograd(N, H):
    x, v, W, b, cot = hp.case(N, H, seed=3)
    t = [torch.tensor(a, requires_grad=True) for a in (x, v, W, b)]
    out = _torch_phi_mean(*t)
    # deepsets_state itself with rho = identity is the same expression
    ident = {"W1": t[2], "b1": t[3], "W2": torch.eye(H, dtype=torch.float64), "b2": torch.zeros(H, dtype=torch.float64)}
    assert torch.equal(hpp.deepsets_state(ident, (t[0], t[1]), L), out @ torch.eye(H, dtype=torch.float64))
    g = torch.autograd.grad((out * torch.tensor(cot)).sum(), t)
    q, u = hp.features(x, v, L, 1.0)
    sx, sv, sp = hp.vjp_scales(W, cot, u, N, L, 1.0)
    ef = np.max(np.abs(hp.forward(x, v, W, b, L) - out.detach().numpy()) / hp.forward_scale(W, b, u, "tanh"))
    mine = hp.vjp(x, v, W, b, cot, L)
    eg = max(np.max(np.abs(m - t_.numpy()) / s) for m, t_, s in zip(mine, g, (sx, sv, sp[:, None], sp)))
    record_measure(f"pool_restatement_vs_torch_forward_N{N}_H{H}", ef)
    record_measure(f"pool_restatement_vs_torch_vjp_N{N}_H{H}", eg)
    # torch's float64 is as far from the longdouble twin as the restatement is: twice the bound covers their difference
    assert ef < 2 * hp.bound("forward", N) and eg < 2 * hp.bound("vjp", N), (ef, eg)


# ---- 2. the floor ---------------------------------------------------------------------------------------------------------------
def test_floor_against_the_longdouble_twin():
    fl = hp.floor()
    record_measure("pool_floor_forward", fl["forward"])
    record_measure("pool_floor_vjp", fl["vjp"])
    # float64 rounding of about H-independent depth plus the unit's resolution at N = 8193 (2 N 2^-61 = 7e-15): anything far above
    # means the restatement and its twin have parted
    assert 0 < fl["forward"] < 1e-13 and 0 < fl["vjp"] < 1e-13, fl


# ---- 3. the hand VJP against central differences -----------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,tol", [("tanh", 1e-7), ("relu", 1e-4)])
def test_hand_vjp_matches_central_differences(activation, tol):
    """eps = 1e-6: the differences of two float64 results (1e-15 of an O(1) value) give 1e-9 and the truncation eps^2 less; for
    relu the particles within eps of a kink, a fraction of order eps of them, carry the wrong slope: 1e-6.  100 x each."""
    x, v, W, b, cot = hp.case(501, 5, seed=11)
    fwd = lambda *a: hp.forward(*a, L, activation)
    grad = lambda *a: hp.vjp(*a, cot, L, activation)
    errs = [hp.fd_error(fwd, grad, x, v, W, b, cot, 1e-6, seed) for seed in range(3)]
    record_measure(f"pool_restatement_fd_{activation}", max(errs))
    assert max(errs) < tol, errs


def test_restatement_is_order_free_and_scales_by_powers_of_two():
    x, v, W, b, cot = hp.case(1000, 5, seed=5)
    perm = np.random.default_rng(0).permutation(1000)
    for activation in ("tanh", "relu"):
        assert np.array_equal(hp.forward(x, v, W, b, L, activation), hp.forward(x[perm], v[perm], W, b, L, activation))
        g, gp = hp.vjp(x, v, W, b, cot, L, activation), hp.vjp(x[perm], v[perm], W, b, cot, L, activation)
        assert np.array_equal(g[0][perm], gp[0]) and np.array_equal(g[2], gp[2]) and np.array_equal(g[3], gp[3])
        gs = hp.vjp(x, v, W, b, cot * 2.0 ** 300, L, activation)
        assert all(np.array_equal(a * 2.0 ** 300, c) for a, c in zip(g, gs))


# ---- 4. the work block's layout ---------------------------------------------------------------------------------------------------
TABLE = [
    # a device forward of the stored particles: the max words and H sums per environment, nothing else
    (f"2 1000 32 {_flags()}", "ok pool=768 max=0 acc=256 gE=null params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # a device VJP with shared parameters: 4H sums, and the rows the reduction over environments reads
    (f"2 1000 32 {_flags(vjp=1, g_x=1, g_v=1, g_params=1)}",
     "ok pool=4352 max=0 acc=256 gE=2304 params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # ... with per-environment parameters the sums go straight to the caller
    (f"2 1000 32 {_flags(vjp=1, per_env=1, g_params=1)}",
     "ok pool=2304 max=0 acc=256 gE=null params=null x=null v=null cot=null out=null g_x=null g_v=null g=null"),
    # a host VJP that gives and wants everything: E N 8 = 16000 bytes round up to 16128
    (f"2 1000 32 {_flags(vjp=1, host=1, params_host=1, xv=1, g_x=1, g_v=1, g_params=1)}",
     "ok pool=71424 max=0 acc=256 gE=2304 params=4352 x=5376 v=21504 cot=37632 out=null g_x=38144 g_v=54272 g=70400"),
    # a host forward with one environment, one particle, one unit
    (f"1 1 1 {_flags(host=1, params_host=1, xv=1)}",
     "ok pool=1536 max=0 acc=256 gE=null params=512 x=768 v=1024 cot=null out=1280 g_x=null g_v=null g=null"),
]


def test_pool_parts_table_and_model(drivers):
    import itertools
    plain, sanitized = drivers
    for cfg, want in TABLE:
        E, N, H, f = map(int, cfg.split())
        assert want == _model(E, N, H, f), cfg              # (the table pins the model, the model the sweep)
    lines = [f"{E} {N} {H} {f}" for E, N, H, f in itertools.product((1, 3, 300), (1, 63, 8193), (1, 5, 33, 256), range(256))]
    lines = [cfg for cfg, _ in TABLE] + lines
    for run in (plain, sanitized):
        got = run(lines)
        for cfg, g in zip(lines, got):
            E, N, H, f = map(int, cfg.split())
            assert g == _model(E, N, H, f), cfg


# ---- 5. the Python argument checks need no device ---------------------------------------------------------------------------------
def _bare_env(E=2, N=10):
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC.__new__(BatchedPIC)            # no handle: a check that reached the library would raise AttributeError
    env.num_envs, env.N = E, N
    return env


@pytest.mark.parametrize("kw,msg", [
    (dict(W=np.zeros((4, 2))), "W must be"),
    (dict(W=np.zeros((3, 4, 3))), "W must be"),
    (dict(W=np.zeros((0, 3)), b=np.zeros(0)), "H must be 1..256"),
    (dict(W=np.zeros((257, 3)), b=np.zeros(257)), "H must be 1..256"),
    (dict(b=np.zeros(5)), "b must have shape"),
    (dict(W=np.zeros((2, 4, 3)), b=np.zeros(4)), "b must have shape"),
    (dict(activation="gelu"), "activation must be"),
    (dict(x=np.zeros((2, 10))), "both be given"),
    (dict(x=np.zeros((2, 9)), v=np.zeros((2, 9))), "x must be"),
    (dict(x=np.zeros((2, 10)), v=np.zeros((10,))), "v must be"),
    (dict(v_scale=float("inf")), "v_scale must be finite"),
])
def test_argument_checks_raise_before_the_device(kw, msg):
    env = _bare_env()
    args = dict(W=np.zeros((4, 3)), b=np.zeros(4))
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        env.pool(**args)
    with pytest.raises(ValueError, match=msg):
        env.pool_vjp(cot=np.zeros((2, np.shape(args["b"])[-1])), **args)


def test_cotangent_shape_is_checked_before_the_device():
    env = _bare_env()
    for cot in (np.zeros((2, 5)), np.zeros(4), np.zeros((3, 4))):
        with pytest.raises(ValueError, match="cot must be"):
            env.pool_vjp(np.zeros((4, 3)), np.zeros(4), cot)
    with pytest.raises(ValueError, match="cot must be"):
        env.pool_vjp(np.zeros((4, 3)), np.zeros(4), None)


def test_header_abi_and_exports_agree():
    import ctypes
    from ocplasma_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    flat = " ".join(hdr.split())
    assert ("typedef struct pic_pool_spec { int32_t hidden, activation, per_env, params_mem_kind; double v_scale; const double* params; } "
            "pic_pool_spec;") in flat
    assert "int pic_pool(pic_handle* h, const pic_pool_spec* s, const void* x, const void* v, int mem_kind, double* out);" in flat
    assert [n for n, _ in _abi.PicPoolSpec._fields_] == ["hidden", "activation", "per_env", "params_mem_kind", "v_scale", "params"]
    assert ctypes.sizeof(_abi.PicPoolSpec) == 4 * 4 + 8 + 8
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _abi.SIGNATURES["pic_pool"] == [vp, ctypes.POINTER(_abi.PicPoolSpec), vp, vp, ci, vp]
    assert _abi.SIGNATURES["pic_pool_vjp"] == [vp, ctypes.POINTER(_abi.PicPoolSpec), vp, vp, vp, ci, vp, vp, vp]
    assert "#define PICSTEP_ABI_VERSION 5" in flat and _abi.ABI_VERSION == 5


# ---- 6. the passes' launch plan ---------------------------------------------------------------------------------------------------
PLAN_TABLE = [
    # E, N, nchunks, wpe, chunks_per_wg, workgroups
    (3, 8193, 9, 9, 1, 9),              # the largest shapes of tests/test_gpu_pool.py: one chunk per workgroup, all of them
    (300, 4097, 5, 5, 1, 5),
    (2, 3000, 3, 3, 1, 3),
    (64, 1000000, 977, 64, 16, 62),     # the workload of profiles/pool_cost.md
    (4096, 1025, 2, 1, 2, 1),           # tests/test_gpu_pool_edges.py: the smallest shapes with a second chunk
    (4096, 2561, 3, 1, 3, 1),
    (1366, 3075, 4, 3, 2, 2),
    (300, 20001, 20, 14, 2, 10),
    (1, 1, 1, 1, 1, 1),
    (1, 1025, 2, 2, 1, 2),
    (5000, 1024, 1, 1, 1, 1),
]


def test_pool_plan_table_and_mirror(drivers):
    import itertools
    for E, N, nchunks, wpe, cpw, wgs in PLAN_TABLE:
        assert hp.plan(E, N) == {"nchunks": nchunks, "wpe": wpe, "chunks_per_wg": cpw, "workgroups": wgs}, (E, N)
    shapes = [(E, N) for E, N, *_ in PLAN_TABLE]
    shapes += list(itertools.product((1, 2, 3, 64, 300, 1365, 1366, 2048, 4095, 4096, 4097, 100000),
                                     (1, 2, 1023, 1024, 1025, 2048, 2049, 2561, 3075, 8193, 20001, 1000000, 2 ** 31 + 1)))
    lines = [f"plan {E} {N}" for E, N in shapes]
    for run in drivers:
        for (E, N), got in zip(shapes, run(lines)):
            p = hp.plan(E, N)
            assert got == f"ok chunks_per_wg={p['chunks_per_wg']} workgroups={p['workgroups']}", (E, N)
            # the workgroups cover every chunk, and none of them is empty
            assert p["workgroups"] * p["chunks_per_wg"] >= p["nchunks"] > (p["workgroups"] - 1) * p["chunks_per_wg"], (E, N)


# ---- 7. the edge tests' preconditions and their exact claims, on the restatement ----------------------------------------------------
def test_restatement_alone_is_inside_the_bound_at_every_scale_set():
    """tests/test_gpu_pool_edges.py compares the device with the twin under hp.bound at other v_scale and L than the floor was
    taken at: the restatement alone must be inside the bound there, or the bound would not be the device's to miss."""
    worst = {"forward": 0.0, "vjp": 0.0}
    for Lb, s, N, H in hp.BOUND_SETS:
        X, V, W, b, cot = hp.scale_case(Lb, s, N, H)
        Wp, bp = np.broadcast_to(W, (2, H, 3)), np.broadcast_to(b, (2, H))
        for act in ("tanh", "relu"):
            out, g = hp.restated(X, V, Wp, bp, cot, Lb, act, s)
            ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, Lb, act, s)
            assert ef < hp.bound("forward", N) and eg < hp.bound("vjp", N), (Lb, s, N, act, ef, eg)
            worst["forward"], worst["vjp"] = max(worst["forward"], ef), max(worst["vjp"], eg)
    record_measure("pool_edges_restatement_forward", worst["forward"])
    record_measure("pool_edges_restatement_vjp", worst["vjp"])


def _eq(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_restatement_v_scale_is_exact_for_powers_of_two_and_zero(act):
    X, V, W, b, cot = hp.scale_case(L, 1.0, 1025, 5)
    for s in hp.V_SCALES_EXACT:
        o1, g1 = hp.restated(X, V, W, b, cot, L, act, s)
        o2, g2 = hp.restated(X, s * V, W, b, cot, L, act, 1.0)
        assert _eq(o1, o2) and all(_eq(g1[k], g2[k]) for k in ("g_x", "g_W", "g_b")) and _eq(g1["g_v"], s * g2["g_v"]), s
    o0, g0 = hp.restated(X, V, W, b, cot, L, act, 0.0)
    oz, gz = hp.restated(X, np.zeros_like(V), W, b, cot, L, act, 1.0)
    assert _eq(o0, oz) and _eq(g0["g_x"], gz["g_x"]) and _eq(g0["g_W"][:, :2], gz["g_W"][:, :2]) and _eq(g0["g_b"], gz["g_b"])
    assert np.all(g0["g_v"] == 0) and np.all(g0["g_W"][:, 2] == 0)


def test_restatement_activation_edges():
    """The exact claims of the device's activation-edge tests hold for the contract as restated, and the restatement stays
    inside the bound at those inputs."""
    E, N, H = hp.EDGE_E, hp.EDGE_N, hp.EDGE_H
    X, _ = hp.box_data(E, N, seed=23)
    W, b = hp.edge_layer()
    Wp, bp, cot = np.broadcast_to(W, (E, H, 3)).copy(), np.broadcast_to(b, (E, H)).copy(), hp.edge_cot()
    fb, vb = hp.bound("forward", N), hp.bound("vjp", N)
    # relu's kink
    outs = []
    for scale in (1.0, 2.0):
        V, s = hp.kink_velocities(scale)
        out, g = hp.restated(X, V, Wp, bp, cot, L, "relu", s)
        ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, L, "relu", s)
        assert ef < fb and eg < vb, (scale, ef, eg)
        assert _eq(out[0, 0], 0.0) and _eq(g["g_b"][0, 0], 0.0)
        outs.append(out)
    assert _eq(*outs)
    # tanh's saturation
    V = hp.saturating_velocities()
    out, g = hp.restated(X, V, Wp, bp, cot, L, "tanh")
    ef, eg = hp.batch_errors(out, g, X, V, Wp, bp, cot, L, "tanh")
    assert ef < fb and eg < vb, (ef, eg)
    assert _eq(out[0, 1], float(np.sum(np.sign(V[0]))) / N) and _eq(g["g_W"][0, 1], np.zeros(3)) and _eq(g["g_b"][0, 1], 0.0)
    Vh, Wh = V.copy(), Wp.copy()
    Vh[1, 5], Wh[:, 1, 2] = 1e200, 1e200
    with np.errstate(over="ignore"):                  # (z = inf is the case)
        out, _ = hp.restated(X, Vh, Wh, bp, None, L, "tanh", vjp_too=False)
    assert np.isfinite(out).all() and hp.batch_errors(out, None, X, Vh, Wh, bp, None, L, "tanh")[0] < fb
    # B_k = 0: +0, and the other rows as without it
    V = hp.box_data(E, N, seed=23)[1]
    out, g = hp.restated(X, V, Wp, bp, cot, L, "relu")
    rest = [0, 1, 3, 4, 5]
    o5, g5 = hp.restated(X, V, Wp[:, rest], bp[:, rest], cot[:, rest], L, "relu")
    assert _eq(out[:, 2], np.zeros(E)) and _eq(g["g_W"][:, 2], np.zeros((E, 3))) and _eq(g["g_b"][:, 2], np.zeros(E))
    assert _eq(out[:, rest], o5) and _eq(g["g_W"][:, rest], g5["g_W"]) and _eq(g["g_b"][:, rest], g5["g_b"])
    assert _eq(g["g_x"], g5["g_x"]) and _eq(g["g_v"], g5["g_v"])
