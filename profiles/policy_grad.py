"""Cost of the stepwise reverse walk: ms per step of pic_tape_backward against a walk of the same tape with null
cotangents (T calls of pic_tape_walk_step plus walk_end, device memory, on torch's stream), at config 2's shape (64 x N = 1e6,
Ng = 256, T = 20) and at the reference's (64 x N = 5000, Ng = 250, T = 100); and the wall time of one forward + backward
training iteration of each policy of examples/policy_gradient.py at the reference's shape.  One JSON line per measurement.

    python profiles/policy_grad.py [--what walk|train|both] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402

SHAPES = {"cfg2": (64, 1_000_000, 256, 20), "ref": (64, 5000, 250, 100)}
M = 5


def _best(fn, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def walk_vs_backward(name, reps):
    E, N, Ng, T = SHAPES[name]
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(E_field(50.0, Ng, M))
    env.use_torch_stream()
    env.start_tape(T, 0)
    env.step_actions_traj(np.random.default_rng(0).uniform(-0.5, 0.5, (T, E, 2 * M)))
    f64 = dict(dtype=torch.float64, device="cuda")
    outs = [torch.empty((T, E, Ng), **f64), torch.empty((T, E, 2 * M), **f64), torch.empty((E, N), **f64), torch.empty((E, N), **f64)]

    def mono():
        env._h.tape_backward_device(0, 0, 0, *(o.data_ptr() for o in outs))

    def walk():
        w = env.walk(M, on_device=True)
        for _ in range(T):
            w.step()
        env._h.tape_walk_end(0, 0, 0, 1, outs[2].data_ptr(), outs[3].data_ptr())
    res = {"what": "walk_vs_backward", "shape": name, "E": E, "N": N, "Ng": Ng, "T": T, "schedule": env._h.schedule()}
    for k, fn in (("backward", mono), ("walk", walk), ("backward", mono), ("walk", walk)):     # interleaved
        ms = 1e3 * _best(fn, reps) / T
        res[f"{k}_ms_per_step"] = min(ms, res.get(f"{k}_ms_per_step", ms))
    res["walk_over_backward"] = res["walk_ms_per_step"] / res["backward_ms_per_step"]
    env.stop_tape()
    env.close()
    print(json.dumps(res), flush=True)


def train(kind, reps, steps=100):
    import policy_gradient as pg
    E, N, Ng, _ = SHAPES["ref"]
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.set_actuator(E_field(50.0, Ng, M))
    env.use_torch_stream()
    policy = pg.make(kind, 50.0, M, 8)
    it = lambda: pg.iteration(env, policy, kind, steps, 8, 0.1, 50.0, 3)
    it()
    s = _best(it, reps)
    env.stop_tape()
    env.close()
    print(json.dumps({"what": "train_iteration", "policy": kind, "E": E, "N": N, "Ng": Ng, "T": steps, "s": s,
                      "ms_per_step": 1e3 * s / steps}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="both", choices=("walk", "train", "both"))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.what in ("walk", "both"):
        for name in ("cfg2", "ref"):
            walk_vs_backward(name, a.reps)
    if a.what in ("train", "both"):
        for kind in ("modes", "state"):
            train(kind, a.reps)
