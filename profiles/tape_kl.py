"""Cost of the per-step KL on the tape: ms per step of the taped forward and of the backward, without a KL, with
the KL recorded but no cotangent on it, and with a cotangent on every step's KL, at config 2's shape and at the reference's, on
64 x 64 and 250 x 250 bins.  As profiles/adjoint_cost.py: wall time per step, best of `reps`, cotangents and outputs in device
memory.  One JSON line per shape and grid; the "plain" figures are adjoint_cost.py's.

    python profiles/tape_kl.py [--shape cfg2|ref|both] [--reps 3]
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
from ocplasma_amd import _abi  # noqa: E402

SHAPES = {"cfg2": (64, 1_000_000, 256, 20), "ref": (64, 5000, 250, 100)}
GRIDS = (64, 250)
VMIN, VMAX = -8.0, 8.0


def measure(E, N, Ng, T, reps):
    import torch
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.set_actuator(E_field(50.0, Ng, 3))
    rng = np.random.default_rng(0)
    a = rng.uniform(-0.5, 0.5, (T, E, 6))
    f64 = dict(dtype=torch.float64, device=torch.device("cuda"))
    cot = torch.tensor(rng.standard_normal((T, 3, E)), **f64)
    ckl = torch.tensor(rng.standard_normal((T, E)), **f64)
    g_ext, g_act = torch.empty((T, E, Ng), **f64), torch.empty((T, E, 6), **f64)
    g_x0, g_v0 = torch.empty((E, N), **f64), torch.empty((E, N), **f64)
    torch.cuda.synchronize()

    def backward():
        env._h.tape_backward_device(cot.data_ptr(), 0, 0, g_ext.data_ptr(), g_act.data_ptr(), g_x0.data_ptr(), g_v0.data_ptr())
        env.sync()

    def case(kl, rows):
        tp, bw = [], []
        for r in range(reps + 1):
            env.reset_sampled("bump-on-tail", seed=1)
            env.start_tape(T, kl=kl)
            env.sync()
            t0 = time.perf_counter()
            env.step_actions_traj(a)
            env.sync()
            t1 = time.perf_counter()
            if rows:
                env._h.tape_kl_cot(ckl.data_ptr(), _abi.PIC_DEVICE, 0, T)
                env.sync()
            t2 = time.perf_counter()
            backward()
            t3 = time.perf_counter()
            st = env.tape_stats()
            env.stop_tape()
            if r:                               # the first round warms up
                tp.append((t1 - t0) / T * 1e3)
                bw.append((t3 - t2) / T * 1e3)
        return {"taped_ms_per_step": min(tp), "backward_ms_per_step": min(bw), "launches": st["launches"],
                "tape_gbytes": st["bytes"] / 1e9, "replay_mismatches": st["replay_mismatches"]}

    out = {"envs": E, "N": N, "Ng": Ng, "T": T, "schedule": env._h.schedule(), "plain": case(None, False)}
    env.reset_sampled("bump-on-tail", seed=1)
    for nb in GRIDS:
        kl = dict(feq=env.phase_density_smooth(nb, VMIN, VMAX), vmin=VMIN, vmax=VMAX)
        out[f"kl_{nb}x{nb}_no_cotangent"] = case(kl, False)
        out[f"kl_{nb}x{nb}"] = case(kl, True)
    out["grad_finite"] = bool(torch.isfinite(g_act).all())
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["cfg2", "ref", "both"])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for name in (("cfg2", "ref") if args.shape == "both" else (args.shape,)):
        print(json.dumps({"shape": name, **measure(*SHAPES[name], args.reps)}), flush=True)
