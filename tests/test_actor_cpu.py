"""The particle actor without a GPU (pic_actor_eval, pic_step_actor): the NumPy restatement of the head
(tests/hp_actor.py) against torch layers, the floors the tolerances rest on, the reference's actor (g20) against the restated
chain, the layout of the call block through a stand-alone C++ driver (plain and under the address and undefined-behaviour
sanitizers), ParticleActor's packing, the Python argument checks, and the compiler's resource report."""
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import hp_actor as ha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimal-control-1d-electrostatic-plasma_amd", "csrc")


# ---- 1. the restatement against torch layers ----------------------------------------------------------------------------------------
def _torch_head(c, params):
    import torch
    import torch.nn as nn
    mods, layers = [], ha.layers_of(c["widths"], c["layernorm"], params)
    for l, (W, b, g, be) in enumerate(layers):
        lin = nn.Linear(W.shape[1], W.shape[0], dtype=torch.float64)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.ascontiguousarray(W)))
            lin.bias.copy_(torch.from_numpy(np.ascontiguousarray(b)))
        mods.append(lin)
        if l + 1 == len(layers):
            break
        if g is not None:
            norm = nn.LayerNorm(W.shape[0], eps=c["ln_eps"], dtype=torch.float64)
            with torch.no_grad():
                norm.weight.copy_(torch.from_numpy(np.ascontiguousarray(g)))
                norm.bias.copy_(torch.from_numpy(np.ascontiguousarray(be)))
            mods.append(norm)
        mods.append(nn.Tanh() if c["activation"] == "tanh" else nn.ReLU())
    return nn.Sequential(*mods)


@pytest.mark.parametrize("case", ha.EVAL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_restatement_against_torch_layers(case):
    """torch sums in another order, so the two float64 evaluations differ like the restatement and its longdouble twin do:
    within 100 x the floor over the same cases."""
    import torch
    c = ha.eval_case(*case)
    u, a = ha.forward(**c)
    E = u.shape[0]
    with torch.no_grad():
        for e in range(E):
            p = c["params"][e] if c["params"].ndim == 2 else c["params"]
            z = _torch_head(c, p)(torch.from_numpy(c["features"][e:e + 1])).numpy()[0]
            want_u = z + c["std"] * c["noise"][e]
            want_a = c["action_shift"] + c["action_scale"] * np.tanh(want_u) if c["squash"] else want_u
            assert np.max(np.abs(u[e] - want_u)) <= 100 * ha.eval_floor(), case
            assert np.max(np.abs(a[e] - want_a)) <= 100 * ha.eval_floor() * ha.action_unit(c), case


# ---- 2. the floors, and the reference's actor -----------------------------------------------------------------------------------------
def test_floors_are_rounding_errors():
    """Both floors are differences of two evaluations of one formula: a few hundred roundings of O(1) values at the most."""
    assert 0 < ha.eval_floor() < 1e-13
    assert 0 < ha.g20_floor() < 1e-13


@pytest.mark.parametrize("pre", ha.G20_CASES)
def test_g20_reference_within_the_floor(pre):
    """The reference's mu = forward(state) and action = sample(state) against the restated chain (pooled features with a
    LayerNorm, then the head) within 100 x the chain's own float64 - longdouble difference over the g20 cases.  Measured:
    floor 1.95e-16; errors (mu, action): a 4.4e-16, 5.6e-16; b 1.1e-16, 1.1e-16; c 5.6e-17, 1.1e-16."""
    e_mu, e_a = ha.g20_reference_error(pre)
    print(f"g20 {pre}: floor {ha.g20_floor():.3g} mu {e_mu:.3g} action {e_a:.3g}")
    assert e_mu <= 100 * ha.g20_floor() and e_a <= 100 * ha.g20_floor()


def test_g20_holds_data_alone():
    g = ha.g20()
    assert os.path.getsize(ha.GOLDEN) < 100 * 1024
    assert all(a.dtype.kind in "fiU" for a in g.values())
    for pre, (E, H, N, M) in zip(ha.G20_CASES, ((1, 16, 513, 3), (2, 5, 64, 1), (2, 5, 64, 1))):
        assert g[f"{pre}_x"].shape == (E, N) and g[f"{pre}_mu"].shape == (E, 2 * M) and int(g[f"{pre}_mlp_dim"]) == H
        L = float(g["L"]) * float(g[f"{pre}_x_norm"])
        assert (g[f"{pre}_x"] < 0).any() and (g[f"{pre}_x"] >= L).any()          # positions partly outside [0, L)
    assert float(g["c_x_norm"]) == 2.0 and (float(g["c_output_min"]), float(g["c_output_max"])) == (-0.5, 2.0)


def test_from_reference_is_the_restated_head():
    from ocplasma_amd.control.actor import ParticleActor
    for pre in ha.G20_CASES:
        g = ha.g20()
        kw, pool = ha.g20_head(pre)
        act = ParticleActor.from_reference(ha.g20_state_dict(pre), L_ref=float(g["L"]), x_norm=float(g[f"{pre}_x_norm"]),
                                           v_norm=float(g[f"{pre}_v_norm"]), output_min=float(g[f"{pre}_output_min"]),
                                           output_max=float(g[f"{pre}_output_max"]))
        assert act.widths == kw["widths"] and np.array_equal(act.params, kw["params"])
        assert (act.action_scale, act.action_shift, act.period, act.v_scale) == (kw["action_scale"], kw["action_shift"], pool["period"],
                                                                                 pool["v_scale"])
        assert act.layernorm and act.squash and act.activation == "relu" and np.array_equal(act.gamma, pool["gamma"])
        # the PPO actor names its last layer fc_pi
        ppo = {k.replace("fc_out", "fc_pi"): a for k, a in ha.g20_state_dict(pre).items()}
        assert np.array_equal(ParticleActor.from_reference(ppo).params, kw["params"])


# ---- 3. ParticleActor's packing ---------------------------------------------------------------------------------------------------------
def _actor(H=5, head=(7, 4), layernorm=True, pool_ln=True, seed=0, **kw):
    from ocplasma_amd.control.actor import ParticleActor
    rng = np.random.default_rng(seed)
    widths = [H, *head]
    ln = dict(gamma=rng.uniform(-1.5, 1.5, H), beta=rng.uniform(-1, 1, H)) if pool_ln else {}
    return ParticleActor(rng.normal(size=(H, 3)), rng.normal(size=H), widths, ha.make_params(widths, layernorm, seed), "relu",
                         layernorm=layernorm, **ln, **kw)


def test_pack_unpack_stack_with_params():
    from ocplasma_amd.control.actor import ParticleActor, head_param_count
    a = _actor()
    assert a.n_params == ha.param_count(a.widths, True) == head_param_count(a.widths, True)
    layers = a.unpack()
    assert [t[2] is not None for t in layers] == [True, False]
    assert np.array_equal(ParticleActor.pack(layers), a.params) and ParticleActor.widths_of(layers) == a.widths
    for got, want in zip(layers, ha.layers_of(a.widths, True, a.params)):
        assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(got, want))
    b = a.with_params(2 * a.params, W=a.W + 1)
    assert np.array_equal(b.params, 2 * a.params) and np.array_equal(b.W, a.W + 1) and np.array_equal(b.b, a.b)
    s = ParticleActor.stack([_actor(seed=0), _actor(seed=1), _actor(seed=2)])
    assert s.per_env and s.params.shape == (3, a.n_params) and s.W.shape == (3, 5, 3) and s.gamma.shape == (3, 5)
    assert np.array_equal(s.unpack()[0][0][1], _actor(seed=1).unpack()[0][0])
    with pytest.raises(ValueError, match="stack"):
        ParticleActor.stack([_actor(), _actor(layernorm=False)])
    with pytest.raises(ValueError, match="do not chain"):
        ParticleActor(a.W, a.b, [6, 4], np.zeros(28))
    with pytest.raises(ValueError, match="params must be"):
        ParticleActor(a.W, a.b, [5, 4], np.zeros(25))
    with pytest.raises(ValueError, match="1..6 linear layers"):
        ParticleActor(a.W, a.b, [5] * 8, np.zeros(1))
    with pytest.raises(ValueError, match="ln_eps"):
        _actor(ln_eps=0.0)
    with pytest.raises(ValueError, match="gamma and beta"):
        ParticleActor(a.W, a.b, [5, 4], np.zeros(24), gamma=np.ones(5))


def test_spec_is_the_c_struct():
    from ocplasma_amd import _abi
    from ocplasma_amd.env._arrays import Mem
    vp, ci = _abi.C.c_void_p, _abi.C.c_int
    assert _abi.SIGNATURES["pic_actor_eval"] == [vp, _abi.C.POINTER(_abi.PicActor), vp, vp, vp, vp, vp, ci, vp, vp, vp]
    assert _abi.SIGNATURES["pic_step_actor"] == [vp, _abi.C.POINTER(_abi.PicActor), vp, vp, ci, ci, vp, vp, vp, vp]
    mem = Mem(0, False, False)
    a = _actor(squash=True, action_scale=1.25, action_shift=0.75)
    s, keep = a.spec(mem, 2)
    assert not s.pool and s.pool_ln.contents.hidden == 5 and s.pool_ln.contents.eps == 1e-5
    assert (s.n_layers, list(s.width), s.layernorm, s.squash, s.per_env) == (2, [5, 7, 4, 0, 0, 0, 0], 1, 1, 0)
    assert (s.ln_eps, s.action_scale, s.action_shift) == (1e-5, 1.25, 0.75)
    assert s.params == keep[2].__array_interface__["data"][0] and s.pool_ln.contents.params == keep[1].__array_interface__["data"][0]
    assert np.array_equal(keep[1], np.concatenate([a.W.ravel(), a.b, a.gamma, a.beta]))
    s, keep = _actor(pool_ln=False).spec(mem, 2)
    assert not s.pool_ln and s.pool.contents.hidden == 5 and keep[1].shape == (20,)
    assert s.activation == s.pool.contents.activation == _abi.PIC_ACT_RELU
    # the head's activation is its own: the per-particle layer keeps `activation`
    mixed = _actor(head_activation="tanh")
    s, keep = mixed.spec(mem, 2)
    assert (s.activation, s.pool_ln.contents.activation) == (_abi.PIC_ACT_TANH, _abi.PIC_ACT_RELU)
    assert mixed.with_params(mixed.params).head_activation == "tanh"
    with pytest.raises(ValueError, match="head_activation must be one of"):
        _actor(head_activation="gelu")


# ---- 4. the layout of the call block ------------------------------------------------------------------------------------------------------
FLAGS = "per_env host stepping particles std noise features_out pre_out actions_out hist".split()


def _build(tmp, name, extra):
    out = str(tmp / name)
    args = ["-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + extra + [os.path.join(ROOT, "tests", "actor_driver.cpp"), "-o", out]
    cxx = shutil.which("c++")
    if cxx:
        cmd = [cxx] + args
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no host C++ compiler (c++ or hipcc) to build tests/actor_driver.cpp with")
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


def _model(E, M, H, P, T, f):
    """The layout restated: the parts in order, each rounded up to 256 bytes; a part without elements has no view."""
    on = {k: bool(f >> i & 1) for i, k in enumerate(FLAGS)}
    frow, arow = E * H, E * 2 * M
    to_caller = not on["host"] and on["features_out"]
    feat = (not to_caller) if on["particles"] else (on["host"] and on["features_out"])
    parts = [("d_act", T * arow if on["stepping"] else (arow if on["host"] and on["actions_out"] else 0)),
             ("d_feat", T * frow if feat else 0), ("d_hist", T * 3 * E if on["hist"] else 0)]
    if on["host"]:
        parts += [("d_params", (E if on["per_env"] else 1) * P), ("d_std", 2 * M if on["std"] else 0),
                  ("d_noise", T * arow if on["noise"] else 0), ("d_features", 0 if on["particles"] else frow),
                  ("d_pre_out", T * arow if on["pre_out"] else 0)]
    else:
        parts += [(k, 0) for k in ("d_params", "d_std", "d_noise", "d_features", "d_pre_out")]
    at, views, spans = 0, [], []
    for name, count in parts:
        views.append(f"{name}={at if count else 'null'}")
        if count:
            spans.append((at, at + 8 * count))
        at = (at + 8 * count + 255) // 256 * 256
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] <= at)      # overlap-free, inside
    return f"ok actor={at} " + " ".join(views)


def test_actor_parts_plain_and_sanitized(tmp_path):
    plain = _build(tmp_path, "actor_driver", [])
    sanitized = _build(tmp_path, "actor_driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    # a pinned row: 3 environments, M = 2, H = 5, P = 100, 4 steps in host memory on particles with every input and output
    pinned = f"3 2 5 100 4 {sum(1 << i for i, k in enumerate(FLAGS) if k != 'per_env')}"
    assert plain([pinned]) == ["ok actor=3840 d_act=0 d_feat=512 d_hist=1024 d_params=1536 d_std=2560 d_noise=2816 d_features=null "
                               "d_pre_out=3328"]
    # device memory, 4 steps on particles: the kernel writes the caller's feature rows itself (no d_feat); without features_out
    # the rows that feed the head live in the block; nothing is staged
    f = lambda *names: sum(1 << FLAGS.index(k) for k in names)
    dev = ("stepping", "particles", "std", "noise", "pre_out", "actions_out", "hist")
    assert plain([f"3 2 5 100 4 {f(*dev, 'features_out')}", f"3 2 5 100 4 {f(*dev)}"]) == [
        "ok actor=1024 d_act=0 d_feat=null d_hist=512 d_params=null d_std=null d_noise=null d_features=null d_pre_out=null",
        "ok actor=1536 d_act=0 d_feat=512 d_hist=1024 d_params=null d_std=null d_noise=null d_features=null d_pre_out=null"]
    # one evaluation on given features in host memory: copies of the features, the parameters, std and the three outputs
    assert plain([f"3 2 5 100 1 {f('host', 'std', 'features_out', 'pre_out', 'actions_out')}"]) == [
        "ok actor=2304 d_act=0 d_feat=256 d_hist=null d_params=512 d_std=1536 d_noise=null d_features=1792 d_pre_out=2048"]
    shapes = [(1, 1, 1, 3, 1), (3, 3, 5, 100, 6), (17, 2, 256, 330000, 2), (300, 64, 33, 7, 1)]
    lines = [f"{E} {M} {H} {P} {T} {f}" for (E, M, H, P, T), f in itertools.product(shapes, range(1 << len(FLAGS)))]
    for run in (plain, sanitized):
        got = run(lines)
        for cfg, g in zip(lines, got):
            assert g == _model(*map(int, cfg.split())), cfg


# ---- 5. the Python argument checks need no device ------------------------------------------------------------------------------------
def _bare_env(E=2, N=10, M=2):
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC.__new__(BatchedPIC)            # no handle: a check that reached the library would raise AttributeError
    env.num_envs, env.N, env.max_mode = E, N, M
    return env


@pytest.mark.parametrize("kw,msg", [
    (dict(features=np.zeros((2, 4))), "features must have shape"),
    (dict(features=np.zeros((3, 5))), "features must have shape"),
    (dict(features=np.zeros((2, 5)), x=np.zeros((2, 10)), v=np.zeros((2, 10))), "features must not be given together with x or v"),
    (dict(features=np.zeros((2, 5)), v=np.zeros((2, 10))), "features must not be given together with x or v"),
    (dict(x=np.zeros((2, 10))), "x and v must both be given"),
    (dict(v=np.zeros((2, 10))), "x and v must both be given"),
    (dict(x=np.zeros((2, 9)), v=np.zeros((2, 10))), "x must have shape"),
    (dict(x=np.zeros((2, 10)), v=np.zeros((1, 10))), "v must have shape"),
    (dict(noise=np.zeros((2, 3))), "noise must have shape"),
    (dict(noise=np.zeros((1, 2, 4))), "noise must have shape"),
    (dict(std=np.zeros(3)), "std must have shape"),
])
def test_actor_eval_shapes_are_checked_before_the_device(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _bare_env().actor_eval(_actor(), **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(nsteps=-1), "nsteps must be >= 0"),
    (dict(nsteps=3, noise=np.zeros((2, 2, 4))), "noise must have shape"),
    (dict(nsteps=3, noise=np.zeros((2, 4))), "noise must have shape"),
    (dict(nsteps=3, std=np.zeros((2, 4))), "std must have shape"),
])
def test_step_actor_shapes_are_checked_before_the_device(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _bare_env().step_actor(_actor(), **kw)


def test_actor_and_environment_must_fit():
    from ocplasma_amd.control.actor import ParticleActor
    with pytest.raises(ValueError, match="last width must be 2 max_mode"):
        _bare_env(M=3).actor_eval(_actor())
    three = ParticleActor.stack([_actor(seed=s) for s in range(3)])
    for call in (lambda e: e.actor_eval(three), lambda e: e.step_actor(three, 1)):
        with pytest.raises(ValueError, match="per-environment actor needs parameters for 2 environments"):
            call(_bare_env())


# ---- 6. the compiler's resource report -----------------------------------------------------------------------------------------------
def test_resource_report():
    from ocplasma_amd import _build
    lib = _build.build_library()
    res = json.load(open(os.path.join(os.path.dirname(lib), "libpicstep.resources.json")))
    hits = [v for k, v in res.items() if "12actor_kernelE" in k]
    assert len(hits) == 1
    assert hits[0]["scratch_bytes_per_lane"] == 0 and hits[0]["agprs"] == 0 and hits[0]["lds_bytes_per_block"] <= 16 * 1024, hits[0]
    # the kernels the calls launch besides, and the policy's and the pool's other kernels: one entry each, zero scratch
    for name in ("policy_kernel", "policy_vjp_kernel", "policy_jvp_kernel", "pool_kernel", "pool_max_kernel", "pool_finish_kernel",
                 "pool_vjp_kernel", "pool_vjp_finish_kernel", "pool_jvp_kernel", "pool_jvp_max_kernel", "pool_jvp_finish_kernel",
                 "pool_ln_kernel", "pool_ln_max_kernel", "pool_ln_finish_kernel", "pool_ln_vjp_kernel", "pool_ln_vjp_finish_kernel",
                 "pool_ln_jvp_kernel", "pool_ln_jvp_max_kernel", "pool_ln_jvp_finish_kernel"):
        hits = [v for k, v in res.items() if f"{len(name)}{name}E" in k]
        assert len(hits) == 1 and hits[0]["scratch_bytes_per_lane"] == 0, name
