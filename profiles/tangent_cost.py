"""Cost of the forward mode of a taped rollout (pic_tape_tangent): ms per step of the tangent in K = 1 and K = 4
directions and of the backward of the same tape, at config 2's shape and at the reference's.  The tangent gets directions on the
actions of every step and on the initial x and v, and writes every output (energy tangents, E_mesh tangents, final x and v) to
device memory; the backward gets cotangents on all three energy traces and on the final x and v.  The timed regions are the
kernels of one call each, no host transfer.  One JSON line per shape.

    python profiles/tangent_cost.py [--shape cfg2|ref|both] [--reps 3] [--once]

--once: one warm-up and one timed call of each kind per shape and nothing else on the device after the tape is made (for a
`rocprofv3 --kernel-trace --stats` run whose statistics should be these calls' kernels plus one taped forward).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402

SHAPES = {"cfg2": (64, 1_000_000, 256, 20), "ref": (64, 5000, 250, 100)}


def measure(E, N, Ng, T, reps, once=False):
    import torch
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.set_actuator(E_field(50.0, Ng, 3))
    rng = np.random.default_rng(0)
    a = rng.uniform(-0.5, 0.5, (T, E, 6))
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    da = torch.randn((4, T, E, 6), generator=gen, **f64)
    dx, dv = torch.randn((4, E, N), generator=gen, **f64), torch.randn((4, E, N), generator=gen, **f64)
    hist, em = torch.empty((4, T, 3, E), **f64), torch.empty((4, T, E, Ng), **f64)
    xo, vo = torch.empty((4, E, N), **f64), torch.empty((4, E, N), **f64)
    cot = torch.tensor(rng.standard_normal((T, 3, E)), **f64)
    g_ext, g_act = torch.empty((T, E, Ng), **f64), torch.empty((T, E, 6), **f64)
    g_x0, g_v0 = torch.empty((E, N), **f64), torch.empty((E, N), **f64)
    torch.cuda.synchronize()

    def tangent(K):
        env._h.tape_tangent_device(K, 0, da.data_ptr(), dx.data_ptr(), dv.data_ptr(), hist.data_ptr(), xo.data_ptr(), vo.data_ptr(),
                                   em.data_ptr())
        env.sync()

    def backward():
        env._h.tape_backward_device(cot.data_ptr(), dx.data_ptr(), dv.data_ptr(), g_ext.data_ptr(), g_act.data_ptr(),
                                    g_x0.data_ptr(), g_v0.data_ptr())
        env.sync()

    def timed(f, *args):
        t0 = time.perf_counter()
        f(*args)
        return (time.perf_counter() - t0) / T * 1e3

    out = {"envs": E, "N": N, "Ng": Ng, "T": T, "directions": "actions of every step, initial x and v",
           "outputs": "device memory (energies, E_mesh, final x and v)"}
    env.reset_sampled("bump-on-tail", seed=1)
    env.start_tape(T)
    env.step_actions_traj(a)
    env.sync()
    runs = {"tangent_k1": [], "tangent_k4": [], "backward": []}
    for r in range(1 if once else reps + 1):
        for K in (1, 4):
            tangent(K)                          # (the first call with K allocates its working memory)
            runs[f"tangent_k{K}"].append(timed(tangent, K))
        backward()
        runs["backward"].append(timed(backward))
    st = env.tape_stats()
    for k, v in runs.items():
        out[f"{k}_ms_per_step"] = float(np.median(v))
    out["k4_over_k1"] = out["tangent_k4_ms_per_step"] / out["tangent_k1_ms_per_step"]
    out["k1_over_backward"] = out["tangent_k1_ms_per_step"] / out["backward_ms_per_step"]
    out["tape_bytes_with_k4"] = st["bytes"]
    out["replay_mismatches"] = st["replay_mismatches"]
    env.stop_tape()
    env.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="both", choices=["cfg2", "ref", "both"])
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--once", action="store_true")
    args = p.parse_args()
    for name in (["cfg2", "ref"] if args.shape == "both" else [args.shape]):
        r = measure(*SHAPES[name], reps=args.reps, once=args.once)
        r["shape"] = name
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
