"""Cost of the gain law: ms per step of pic_step_feedback against pic_step_feedback_gain (G0 and a dense random
G) in one multi-step call, and ms per step of the backward of a gain-law tape against an open-loop tape of the same length (energy cotangents, every output written to device memory), at
the reference's feedback shape (256 x N = 5000, Ng = 250, M = 5: resident schedule) and at config 2's (64 x N = 1e6, Ng = 256,
M = 5: streaming).  One JSON line per shape.

    python profiles/feedback_gain.py [--shape ref|cfg2|both] [--reps 3]
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

SHAPES = {"ref": (256, 5000, 250, 100, 20), "cfg2": (64, 1_000_000, 256, 20, 10)}   # E, N, Ng, forward steps, taped steps
M = 5


def _timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def measure(E, N, Ng, T, Tb, reps):
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(E_field(50.0, Ng, M))
    n = 2 * M
    g0 = np.diag(np.concatenate([-np.ones(M), np.ones(M)]))
    G0 = np.broadcast_to(g0, (E, n, n)).copy()
    Gr = g0 + 0.05 * np.random.default_rng(0).standard_normal((E, n, n))
    out = {"E": E, "N": N, "Ng": Ng, "M": M, "schedule": env._h.schedule(), "steps": T}

    def fwd(kind):
        def run():
            if kind == "law":
                env.step_feedback(T)
            else:
                env.step_feedback_gain(G0 if kind == "g0" else Gr, T)
            env.sync()
        return run
    for kind in ("law", "g0", "dense", "law", "g0", "dense"):        # (interleaved: drift hits all three alike)
        ms = 1e3 * _timed(fwd(kind), reps) / T
        out[f"fwd_{kind}_ms_per_step"] = min(ms, out.get(f"fwd_{kind}_ms_per_step", ms))
    import torch
    rng = np.random.default_rng(1)
    f64 = dict(dtype=torch.float64, device="cuda")
    cot = torch.tensor(rng.standard_normal((Tb, 3, E)), **f64)
    a = rng.uniform(-0.5, 0.5, (Tb, E, n))
    outs = [torch.empty((Tb, E, Ng), **f64), torch.empty((Tb, E, n), **f64), torch.empty((E, N), **f64),
            torch.empty((E, N), **f64), torch.empty((Tb, E, n), **f64)]

    def bwd(kind):
        def run():
            env.stop_tape()
            env.start_tape(Tb)
            if kind == "open":
                env.step_actions_traj(a)
            else:
                env.step_feedback_gain(Gr, Tb)
            env.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env._h.tape_backward_feedback_device(cot.data_ptr(), 0, 0, 0, *(t.data_ptr() for t in outs))
            env.sync()
            return time.perf_counter() - t0
        return run
    for kind in ("open", "law", "open", "law"):
        run = bwd(kind)
        ms = 1e3 * min(run() for _ in range(reps)) / Tb
        out[f"bwd_{kind}_ms_per_step"] = min(ms, out.get(f"bwd_{kind}_ms_per_step", ms))
        st = env.tape_stats()
        assert st["replay_mismatches"] == 0, st
        out[f"tape_{kind}_bytes"] = st["bytes"]
    env.stop_tape()
    env.close()
    out["fwd_g0_over_law"] = out["fwd_g0_ms_per_step"] / out["fwd_law_ms_per_step"]
    out["fwd_dense_over_law"] = out["fwd_dense_ms_per_step"] / out["fwd_law_ms_per_step"]
    out["bwd_law_over_open"] = out["bwd_law_ms_per_step"] / out["bwd_open_ms_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["ref", "cfg2", "both"])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for name in (("ref", "cfg2") if args.shape == "both" else (args.shape,)):
        print(json.dumps({"shape": name, **measure(*SHAPES[name], args.reps)}), flush=True)


if __name__ == "__main__":
    main()
