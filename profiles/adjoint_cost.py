"""Cost of a differentiable rollout: ms per step of the forward untaped, the forward taped (default checkpoint
interval) and the backward, at config 2's shape and at the reference's.  The backward gets cotangents on all three energy traces
and on the final x and v, and writes every output (e-bar, a-bar, x0-bar, v0-bar) to device memory: the timed region is the
backward's kernels, no host transfer.  One JSON line per shape.

    python profiles/adjoint_cost.py [--shape cfg2|ref|both] [--reps 3] [--backward-only]

--backward-only: one warm-up and one timed backward per shape and nothing else on the device after the tape is made (for a
`rocprofv3 --kernel-trace --stats` run whose statistics should be the backward's own kernels plus one taped forward).
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


def measure(E, N, Ng, T, reps, backward_only=False):
    import torch
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.set_actuator(E_field(50.0, Ng, 3))
    rng = np.random.default_rng(0)
    a = rng.uniform(-0.5, 0.5, (T, E, 6))
    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)
    cot = torch.tensor(rng.standard_normal((T, 3, E)), **f64)
    cx = torch.randn((E, N), generator=torch.Generator(device=dev).manual_seed(1), **f64)
    cv = torch.randn((E, N), generator=torch.Generator(device=dev).manual_seed(2), **f64)
    g_ext, g_act = torch.empty((T, E, Ng), **f64), torch.empty((T, E, 6), **f64)
    g_x0, g_v0 = torch.empty((E, N), **f64), torch.empty((E, N), **f64)
    torch.cuda.synchronize()

    def backward():
        env._h.tape_backward_device(cot.data_ptr(), cx.data_ptr(), cv.data_ptr(), g_ext.data_ptr(), g_act.data_ptr(),
                                    g_x0.data_ptr(), g_v0.data_ptr())
        env.sync()

    out = {"envs": E, "N": N, "Ng": Ng, "T": T, "cotangents": "KE, PE, PE_reward of every step; final x and v",
           "outputs": "device memory"}
    if backward_only:
        env.reset_sampled("bump-on-tail", seed=1)
        env.start_tape(T)
        env.step_actions_traj(a)
        env.sync()
        backward()
        t0 = time.perf_counter()
        backward()
        out["backward_ms_per_step"] = (time.perf_counter() - t0) / T * 1e3
        out["replay_mismatches"] = env.tape_stats()["replay_mismatches"]
        env.stop_tape()
        env.close()
        return out
    fw, tp, bw = [], [], []
    for r in range(reps + 1):
        env.reset_sampled("bump-on-tail", seed=1)
        env.sync()
        t0 = time.perf_counter()
        env.step_actions_traj(a)
        env.sync()
        t1 = time.perf_counter()
        env.reset_sampled("bump-on-tail", seed=1)
        env.start_tape(T)
        env.sync()
        t2 = time.perf_counter()
        env.step_actions_traj(a)
        env.sync()
        t3 = time.perf_counter()
        backward()
        t4 = time.perf_counter()
        st = env.tape_stats()
        env.stop_tape()
        if r:                                   # the first round warms up
            fw.append((t1 - t0) / T * 1e3)
            tp.append((t3 - t2) / T * 1e3)
            bw.append((t4 - t3) / T * 1e3)
    out.update(forward_ms_per_step=min(fw), taped_ms_per_step=min(tp), backward_ms_per_step=min(bw),
               backward_over_forward=min(bw) / min(fw), taped_over_forward=min(tp) / min(fw),
               checkpoint_every=st["checkpoint_every"], tape_gbytes=st["bytes"] / 1e9, launches=st["launches"],
               replay_mismatches=st["replay_mismatches"], grad_finite=bool(torch.isfinite(g_act).all()))
    env.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["cfg2", "ref", "both"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--backward-only", action="store_true")
    args = ap.parse_args()
    for name in (("cfg2", "ref") if args.shape == "both" else (args.shape,)):
        print(json.dumps({"shape": name, **measure(*SHAPES[name], args.reps, args.backward_only)}), flush=True)
