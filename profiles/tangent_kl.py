"""Cost of the forward mode of the per-step smoothed KL (pic_tape_tangent_kl): ms per step of tangent(kl=True)
against tangent() on the same tape, interleaved, best of --reps, in K = 1 and K = 4 directions, at config 2's shape and at the
reference's, with 64 x 64 bins on [-6, 6] and the smoothed density of the starting state as the target.  Directions on the actions
of every step and on the initial x and v; every output goes to device memory; the timed regions are the kernels of one call each.
One JSON line per shape.

    python profiles/tangent_kl.py [--shape cfg2|ref|both] [--reps 3] [--once]

--once: one warm-up and one timed call of each kind per shape (for a `rocprofv3 --kernel-trace --stats` run).
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
BINS, VMIN, VMAX = 64, -6.0, 6.0


def measure(E, N, Ng, T, reps, once=False):
    import torch
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.set_actuator(E_field(50.0, Ng, 3))
    rng = np.random.default_rng(0)
    a = rng.uniform(-0.5, 0.5, (T, E, 6))
    f64 = dict(dtype=torch.float64, device=torch.device("cuda"))
    gen = torch.Generator(device="cuda").manual_seed(1)
    da = torch.randn((4, T, E, 6), generator=gen, **f64)
    dx, dv = torch.randn((4, E, N), generator=gen, **f64), torch.randn((4, E, N), generator=gen, **f64)
    hist, em, dkl = torch.empty((4, T, 3, E), **f64), torch.empty((4, T, E, Ng), **f64), torch.empty((4, T, E), **f64)
    xo, vo = torch.empty((4, E, N), **f64), torch.empty((4, E, N), **f64)
    torch.cuda.synchronize()

    def tangent(K, kl):
        env._h._tape_tangent(ocplasma_amd._abi.PIC_DEVICE, K, 0, da.data_ptr(), dx.data_ptr(), dv.data_ptr(), hist.data_ptr(),
                             xo.data_ptr(), vo.data_ptr(), em.data_ptr(), kl=dkl.data_ptr() if kl else None)
        env.sync()

    def timed(*args):
        t0 = time.perf_counter()
        tangent(*args)
        return (time.perf_counter() - t0) / T * 1e3

    env.reset_sampled("bump-on-tail", seed=1)
    feq = env.phase_density_smooth(BINS, VMIN, VMAX)
    env.start_tape(T, kl=dict(feq=feq, vmin=VMIN, vmax=VMAX))
    env.step_actions_traj(a)
    env.sync()
    out = {"envs": E, "N": N, "Ng": Ng, "T": T, "bins": [BINS, BINS], "v_range": [VMIN, VMAX]}
    runs = {(K, kl): [] for K in (1, 4) for kl in (False, True)}
    launches = {}
    for K in (1, 4):
        for kl in (False, True):
            tangent(K, kl)                      # (the first calls allocate the working memory)
            launches[(K, kl)] = env.tape_stats()["launches"]
    for r in range(1 if once else reps):
        for key in runs:
            runs[key].append(timed(*key))
    for K in (1, 4):
        plain, with_kl = min(runs[(K, False)]), min(runs[(K, True)])
        out[f"tangent_k{K}_ms_per_step"] = plain
        out[f"tangent_kl_k{K}_ms_per_step"] = with_kl
        out[f"kl_k{K}_extra_ms_per_step"] = with_kl - plain
        out[f"kl_k{K}_extra_percent"] = 100.0 * (with_kl - plain) / plain
        out[f"launches_k{K}"] = [launches[(K, False)], launches[(K, True)]]
    st = env.tape_stats()
    out["tape_bytes"] = st["bytes"]
    out["replay_mismatches"] = st["replay_mismatches"]
    out["device_memory_allocated_bytes"] = int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0])
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
