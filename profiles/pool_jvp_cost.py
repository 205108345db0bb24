"""Cost of the forward mode of the pooled particle features.  One JSON line per layer and K: median, minimum and
maximum over --reps rounds with the variants interleaved (one warm-up round first), every timing between two device
synchronisations and over --inner calls.  At the reference's shape, 64 x 5000 with H = 32, for K in {1, 4, 8} and both layers:

  one_call:    BatchedPIC.pool_jvp with K directions in one call (tangents of x, v and every parameter)
  k_calls:     K calls of one direction each: what sharing sincos, tanh and the LayerNorm's statistics across a group buys
  torch_f64 / torch_f32: torch.func.jvp of the same layer in torch, once per direction, in float64 and in float32

    python profiles/pool_jvp_cost.py [--reps 5] [--inner 20]
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
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC  # noqa: E402

L, H, E, N, NG = 50.0, 32, 64, 5000, 250
NAMES = ("d_x", "d_v", "d_W", "d_b", "d_gamma", "d_beta")


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


def _torch_layer(ln, x, v, W, b, gamma=None, beta=None):
    q = (2 * math.pi / L) * x
    n = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1).to(W.dtype) @ W.T + b
    if ln:
        return torch.relu(torch.nn.functional.layer_norm(n, (H,), gamma, beta, 1e-5)).mean(dim=-2)
    return torch.tanh(n).mean(dim=-2)


def run(reps, inner):
    env = BatchedPIC(E, N, NG, L=L, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.use_torch_stream()
    views = env._ordered_views()
    x, v = (views[k].clone(memory_format=torch.contiguous_format) for k in ("x", "v"))
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).cuda()              # noqa: E731
    p = [r(H, 3) * 0.5, r(H) * 0.1, 1.0 + 0.3 * r(H), 0.3 * r(H)]
    for ln in (False, True):
        prim = (x, v, *(p if ln else p[:2]))
        act = "relu" if ln else "tanh"
        kw = dict(gamma=p[2], beta=p[3]) if ln else {}
        for K in (1, 4, 8):
            t = {k: r(K, *a.shape) for k, a in zip(NAMES, prim)}

            def one_call():
                return env.pool_jvp(p[0], p[1], activation=act, x=x, v=v, **kw, **t)

            def k_calls():
                return [env.pool_jvp(p[0], p[1], activation=act, x=x, v=v, **kw, **{k: a[kk] for k, a in t.items()}) for kk in range(K)]

            def eager(dtype):
                pd = tuple(a.to(dtype) if i >= 2 else a for i, a in enumerate(prim))
                td = [tuple(a[kk].to(dtype) if i >= 2 else a[kk] for i, a in enumerate(t.values())) for kk in range(K)]
                return lambda: [torch.func.jvp(lambda *a: _torch_layer(ln, *a), pd, td[kk])[1] for kk in range(K)]
            # the results the timings are about agree (float64)
            want = torch.stack(eager(torch.float64)())
            d = float((one_call() - want).abs().max() / want.abs().max())
            assert d < 1e-11 and torch.equal(one_call(), torch.stack(k_calls())), d
            stats = _interleaved({"one_call": one_call, "k_calls": k_calls, "torch_f64": eager(torch.float64),
                                  "torch_f32": eager(torch.float32)}, reps, inner)
            res = {"what": "pool_jvp", "layer": "layernorm" if ln else "plain", "activation": act, "E": E, "N": N, "H": H, "K": K,
                   "reps": reps, "inner": inner, "agrees_with_torch_f64_rel": d}
            for k, s in stats.items():
                res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = (1e3 * a for a in s)
            print(json.dumps(res), flush=True)
    env.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    run(a.reps, a.inner)
