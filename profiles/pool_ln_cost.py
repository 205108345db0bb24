"""Cost of the pooled particle features with a LayerNorm.  One JSON line per measurement: median, minimum and
maximum over --reps rounds with the variants interleaved (one warm-up round first), every timing between two device
synchronisations and over --inner calls.

  op:    pic_pool_ln + pic_pool_ln_vjp (forward + backward through control.pool.pooled_features, gradients for x, v, W, b, gamma,
         beta) against the same layer in torch, mean_i relu(LayerNorm(W (cos q_i, sin q_i, v_i) + b)), in float64 and in float32,
         at the reference's shape (64 x 5000, H = 32) and at config 2's (64 x 1e6; torch there on --torch-envs environments,
         because [E, N, H] of all 64 does not fit next to its backward: its time is scaled to 64 and marked so)
  train: one training iteration (forward + backward, 64 x 5000, T = 100) of examples/pooled_policy.py's loop with --layernorm
         and of the same policy in torch layers, float64

    python profiles/pool_ln_cost.py [--what op|train|both] [--reps 5] [--inner 3] [--torch-envs 4]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.control.pool import pooled_features  # noqa: E402

L, M, H = 50.0, 5, 32
SHAPES = {"ref": (64, 5000, 250), "cfg2": (64, 1_000_000, 256)}


def _time(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def _interleaved(variants, reps, inner):
    """{name: (median, min, max) seconds per call} over `reps` rounds, every round running each variant (one warm-up round)."""
    times = {k: [] for k in variants}
    for r in range(reps + 1):
        for k, fn in variants.items():
            s = _time(fn, inner)
            if r:
                times[k].append(s)
    return {k: (statistics.median(t), min(t), max(t)) for k, t in times.items()}


def _ms(res, key, stats, scale=1.0):
    res[key + "_ms_median"], res[key + "_ms_min"], res[key + "_ms_max"] = (1e3 * scale * s for s in stats)


def _torch_layer(x, v, W, b, gamma, beta):
    q = (2 * math.pi / L) * x
    f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1).to(W.dtype)
    return torch.relu(torch.nn.functional.layer_norm(f @ W.T + b, (H,), gamma, beta, 1e-5)).mean(dim=-2)


def op(name, reps, inner, torch_envs):
    E, N, Ng = SHAPES[name]
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.use_torch_stream()
    views = env._ordered_views()
    x, v = (views[k].clone(memory_format=torch.contiguous_format) for k in ("x", "v"))
    g = torch.Generator().manual_seed(0)
    p64 = [(torch.randn(H, 3, generator=g, dtype=torch.float64) * 0.5), torch.randn(H, generator=g, dtype=torch.float64) * 0.1,
           torch.empty(H, dtype=torch.float64).uniform_(-1.5, 1.5, generator=g), torch.empty(H, dtype=torch.float64).uniform_(-1, 1, generator=g)]
    p64 = [t.cuda().requires_grad_(True) for t in p64]
    cot = torch.randn(E, H, generator=g, dtype=torch.float64).cuda()
    Et = E if name == "ref" else torch_envs
    xs, vs = x[:Et].clone().requires_grad_(True), v[:Et].clone().requires_grad_(True)
    xg, vg = x.clone().requires_grad_(True), v.clone().requires_grad_(True)

    def fused():
        out = pooled_features(env, xg, vg, p64[0], p64[1], "relu", 1.0, p64[2], p64[3])
        torch.autograd.grad((out * cot).sum(), (xg, vg, *p64))

    def eager(dtype):
        p = [t.detach().to(dtype).requires_grad_(True) for t in p64]

        def run():
            out = _torch_layer(xs, vs, *p)
            torch.autograd.grad((out * cot[:Et].to(dtype)).sum(), (xs, vs, *p))
        return run
    # the results the timings are about agree (float64; section 6 of the measuring guide)
    with torch.no_grad():
        a = pooled_features(env, x[:Et], v[:Et], *p64[:2], "relu", 1.0, *p64[2:]) if Et == E else None
        if a is not None:
            d = float((a - _torch_layer(x, v, *[t.detach() for t in p64])).abs().max())
            assert d < 1e-12, d
    stats = _interleaved({"fused_f64": fused, "torch_f64": eager(torch.float64), "torch_f32": eager(torch.float32)}, reps, inner)
    res = {"what": "op_forward_backward", "shape": name, "E": E, "N": N, "H": H, "torch_envs": Et, "reps": reps, "inner": inner}
    _ms(res, "fused_f64", stats["fused_f64"])
    for k in ("torch_f64", "torch_f32"):
        _ms(res, k + "_measured", stats[k])
        _ms(res, k + "_scaled_to_E", stats[k], E / Et)
    env.close()
    print(json.dumps(res), flush=True)


class TorchLnDeepSets(torch.nn.Module):
    """The function of examples/pooled_policy.py --layernorm in torch layers, float64."""

    def __init__(self, max_mode, hidden=H):
        super().__init__()
        self.phi = torch.nn.Sequential(torch.nn.Linear(3, hidden), torch.nn.LayerNorm(hidden), torch.nn.ReLU()).double()
        self.rho = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * max_mode)).double()

    def forward(self, xv):
        x, v = xv
        q = (2 * math.pi / L) * x
        f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1)
        return self.rho(self.phi(f).mean(dim=-2))


def train(reps, steps=100):
    import policy_gradient as pg
    import pooled_policy as pp
    E, N, Ng = SHAPES["ref"]
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.set_actuator(E_field(L, Ng, M))
    env.use_torch_stream()
    policies = {"torch_layernorm_f64": TorchLnDeepSets(M).to("cuda"), "pool_encoder_layernorm_f64": pp.make(env, M, layernorm=True),
                "pool_encoder_plain_f64": pp.make(env, M)}
    stats = _interleaved({k: (lambda p=p: pg.iteration(env, p, "state", steps, 8, 0.1, L, 3)) for k, p in policies.items()}, reps, 1)
    env.stop_tape()
    env.close()
    res = {"what": "train_iteration", "E": E, "N": N, "Ng": Ng, "T": steps, "reps": reps}
    for k, s in stats.items():
        _ms(res, k, s)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=("op", "train", "both"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--torch-envs", type=int, default=4)
    a = ap.parse_args()
    if a.what in ("op", "both"):
        for name in ("ref", "cfg2"):
            op(name, a.reps, a.inner * (20 if name == "ref" else 1), a.torch_envs)     # (a call at `ref` is under a millisecond)
    if a.what in ("train", "both"):
        train(a.reps)
