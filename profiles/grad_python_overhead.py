"""Host time per call of the two per-step entries of the Python differentiation layer, with CUDA-tensor arguments on torch's
stream, at the reference's shape of profiles/policy_grad.py (64 x N = 5000, Ng = 250, max_mode = 5): TapeWalk.step over walks of
a 100-step tape, and BatchedPIC.backward on a 5-step tape.  These are Python-side times (time.perf_counter around the call), not
kernel times: walk.step returns without waiting, backward ends by reading the tape's counters, which waits for its kernels.
One JSON line: the median, and the quartiles, in microseconds.

    python profiles/grad_python_overhead.py [--calls 300] [--root DIR]

--root DIR measures the checkout at DIR instead of this one (two commits in one session, on one machine).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402

E, N, NG, M, T_WALK, T_BACK = 64, 5000, 250, 5, 100, 5


def _env(T):
    env = BatchedPIC(E, N, NG, L=50.0, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(E_field(50.0, NG, M))
    env.use_torch_stream()
    env.start_tape(T, 0)
    env.step_actions_traj(np.random.default_rng(0).uniform(-0.5, 0.5, (T, E, 2 * M)))
    return env


def _stats(us):
    q = np.percentile(np.asarray(us) * 1e6, [25, 50, 75])
    return {"median_us": round(float(q[1]), 2), "q25_us": round(float(q[0]), 2), "q75_us": round(float(q[2]), 2), "calls": len(us)}


def walk_step():
    env = _env(T_WALK)
    g = torch.Generator(device="cuda").manual_seed(0)
    d_en = torch.randn((3, E), dtype=torch.float64, device="cuda", generator=g)
    d_md = torch.randn((E, 2 * M), dtype=torch.float64, device="cuda", generator=g)
    times = []
    for rep in range(1 + -(-args.calls // T_WALK)):              # the first walk warms up
        w = env.walk(M, on_device=True)
        for _ in range(T_WALK):
            t0 = time.perf_counter()
            w.step(d_energies=d_en, d_modes=d_md)
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
        w.end()
        torch.cuda.synchronize()
    env.stop_tape()
    env.close()
    return _stats(times)


def backward():
    env = _env(T_BACK)
    g = torch.Generator(device="cuda").manual_seed(1)
    d_per = torch.randn((T_BACK, E), dtype=torch.float64, device="cuda", generator=g)
    d_x = torch.randn((E, N), dtype=torch.float64, device="cuda", generator=g)
    times = []
    for i in range(20 + args.calls):                             # 20 calls warm up
        t0 = time.perf_counter()
        env.backward(d_PE_reward=d_per, d_x=d_x)
        dt = time.perf_counter() - t0
        if i >= 20:
            times.append(dt)
    env.stop_tape()
    env.close()
    return _stats(times)


if __name__ == "__main__":
    print(json.dumps({"what": "grad_python_overhead", "label": args.label, "walk_step": walk_step(), "backward": backward()}),
          flush=True)
