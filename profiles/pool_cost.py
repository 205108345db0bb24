"""Cost of the pooled particle features.  One JSON line per measurement, best of --reps with the variants
interleaved:

  op:    pic_pool + pic_pool_vjp (forward + backward through control.pool.pooled_features) against the same expression in torch,
         mean_i tanh(W (cos q_i, sin q_i, v_i) + b), in float64 and in float32, at the reference's shape (64 x 5000, H = 32) and
         at config 2's (64 x 1e6; torch there on --torch-envs environments, because [E, N, H] of all 64 does not fit next to its
         backward: its time is scaled to 64 and marked so)
  train: one training iteration (forward + backward, 64 x 5000, T = 100) of examples/policy_gradient.py's DeepSets policy (two
         per-particle layers, float32), of a torch DeepSets with one per-particle layer in float64 (the function PoolEncoder
         computes) and of examples/pooled_policy.py's policy

    python profiles/pool_cost.py [--what op|train|both] [--reps 3] [--torch-envs 4]
"""
import argparse
import json
import math
import os
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


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _interleaved(variants, reps):
    """{name: best seconds} over `reps` rounds, every round running each variant once (one warm-up round first)."""
    best = {k: float("inf") for k in variants}
    for r in range(reps + 1):
        for k, fn in variants.items():
            s = _time(fn)
            if r:
                best[k] = min(best[k], s)
    return best


def _torch_phi_mean(x, v, W, b):
    q = (2 * math.pi / L) * x
    f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1).to(W.dtype)
    return torch.tanh(f @ W.T + b).mean(dim=-2)


def op(name, reps, torch_envs):
    E, N, Ng = SHAPES[name]
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.use_torch_stream()
    views = env._ordered_views()
    x, v = (views[k].clone(memory_format=torch.contiguous_format) for k in ("x", "v"))
    g = torch.Generator().manual_seed(0)
    W64 = (torch.randn(H, 3, generator=g, dtype=torch.float64) * 0.5).cuda().requires_grad_(True)
    b64 = (torch.randn(H, generator=g, dtype=torch.float64) * 0.1).cuda().requires_grad_(True)
    cot = torch.randn(E, H, generator=g, dtype=torch.float64).cuda()
    Et = E if name == "ref" else torch_envs
    xs, vs = x[:Et].clone().requires_grad_(True), v[:Et].clone().requires_grad_(True)
    xg, vg = x.clone().requires_grad_(True), v.clone().requires_grad_(True)

    def fused():
        out = pooled_features(env, xg, vg, W64, b64)
        torch.autograd.grad((out * cot).sum(), (xg, vg, W64, b64))

    def eager(dtype):
        W, b = W64.detach().to(dtype).requires_grad_(True), b64.detach().to(dtype).requires_grad_(True)

        def run():
            out = _torch_phi_mean(xs, vs, W, b)
            torch.autograd.grad((out * cot[:Et].to(dtype)).sum(), (xs, vs, W, b))
        return run
    best = _interleaved({"fused_f64": fused, "torch_f64": eager(torch.float64), "torch_f32": eager(torch.float32)}, reps)
    res = {"what": "op_forward_backward", "shape": name, "E": E, "N": N, "H": H, "torch_envs": Et,
           "fused_f64_ms": 1e3 * best["fused_f64"]}
    for k in ("torch_f64", "torch_f32"):
        res[k + "_ms_measured"] = 1e3 * best[k]
        res[k + "_ms_scaled_to_E"] = 1e3 * best[k] * E / Et
    env.close()
    print(json.dumps(res), flush=True)


class OneLayerDeepSets(torch.nn.Module):
    """The function of examples/pooled_policy.py in torch layers, float64."""

    def __init__(self, max_mode, hidden=H):
        super().__init__()
        self.phi = torch.nn.Linear(3, hidden).double()
        self.rho = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * max_mode)).double()

    def forward(self, xv):
        x, v = xv
        q = (2 * math.pi / L) * x
        f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1)
        return self.rho(torch.tanh(self.phi(f)).mean(dim=-2))


def train(reps, steps=100):
    import policy_gradient as pg
    import pooled_policy as pp
    E, N, Ng = SHAPES["ref"]
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.set_actuator(E_field(L, Ng, M))
    env.use_torch_stream()
    policies = {"example_deepsets_2layer_f32": pg.make("state", L, M, 8), "torch_1layer_f64": OneLayerDeepSets(M).to("cuda"),
                "pool_encoder_f64": pp.make(env, M)}
    best = _interleaved({k: (lambda p=p: pg.iteration(env, p, "state", steps, 8, 0.1, L, 3)) for k, p in policies.items()}, reps)
    env.stop_tape()
    env.close()
    print(json.dumps({"what": "train_iteration", "E": E, "N": N, "Ng": Ng, "T": steps, **{k + "_ms": 1e3 * s for k, s in best.items()}}),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=("op", "train", "both"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-envs", type=int, default=4)
    a = ap.parse_args()
    if a.what in ("op", "both"):
        for name in ("ref", "cfg2"):
            op(name, a.reps, a.torch_envs)
    if a.what in ("train", "both"):
        train(a.reps)
