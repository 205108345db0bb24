"""Host time per call of entries of the Python differentiation layer, with CUDA-tensor arguments on torch's stream, at the
reference's shape of profiles/policy_grad.py (64 x N = 5000, Ng = 250, max_mode = 5): TapeWalk.step over walks of a 100-step tape,
BatchedPIC.backward and BatchedPIC.tangent (one direction without a K axis, and K = 4) on a 5-step tape, and
BatchedPIC.moments_jvp (one direction).  These are Python-side times (time.perf_counter around the call), not kernel times:
walk.step and moments_jvp return without waiting, backward and tangent end by reading the tape's counters, which waits for
their kernels.  One JSON line: the median, and the quartiles, in microseconds.

    python profiles/grad_python_overhead.py [--calls 300] [--root DIR] [--fake]

--root DIR measures the checkout at DIR instead of this one (two commits in one session, on one machine).
--fake needs no GPU and no library: a handle whose every method returns at once stands in for _abi.Handle and the arguments
are NumPy arrays, so that the Python layer is the whole cost.
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
ap.add_argument("--fake", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field, _abi  # noqa: E402

E, N, NG, M, T_WALK, T_BACK = 64, 5000, 250, 5, 100, 5


class _NoHandle:
    """--fake: every Handle method returns at once; the tape holds as many steps as start_tape allowed."""
    fixed_positions = False

    def __init__(self, *a):
        self.steps = 0

    def tape_start(self, max_steps, *a):
        self.steps = max_steps

    def tape_stats(self):
        return {"steps": self.steps, "replay_mismatches": 0}

    def tape_law_calls(self):
        return []

    def __getattr__(self, name):
        return lambda *a, **k: 0


def _randn(shape, seed):
    if args.fake:
        return np.random.default_rng(seed).standard_normal(shape)
    return torch.randn(shape, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _env(T):
    if args.fake:
        _abi.Handle = _NoHandle
    env = BatchedPIC(E, N, NG, L=50.0, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(E_field(50.0, NG, M))
    if not args.fake:
        env.use_torch_stream()
    env.start_tape(T, 0)
    env.step_actions_traj(np.random.default_rng(0).uniform(-0.5, 0.5, (T, E, 2 * M)))
    return env


def _time(call, warm=20):
    times = []
    for i in range(warm + args.calls):                           # `warm` calls warm up
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= warm:
            times.append(dt)
    return _stats(times)


def _stats(us):
    q = np.percentile(np.asarray(us) * 1e6, [25, 50, 75])
    return {"median_us": round(float(q[1]), 2), "q25_us": round(float(q[0]), 2), "q75_us": round(float(q[2]), 2), "calls": len(us)}


def walk_step():
    env = _env(T_WALK)
    d_en, d_md = _randn((3, E), 0), _randn((E, 2 * M), 1)
    times = []
    for rep in range(1 + -(-args.calls // T_WALK)):              # the first walk warms up
        w = env.walk(M, on_device=not args.fake)
        for _ in range(T_WALK):
            t0 = time.perf_counter()
            w.step(d_energies=d_en, d_modes=d_md)
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
        w.end()
        if not args.fake:
            torch.cuda.synchronize()
    env.stop_tape()
    env.close()
    return _stats(times)


def backward():
    env = _env(T_BACK)
    d_per, d_x = _randn((T_BACK, E), 2), _randn((E, N), 3)
    out = _time(lambda: env.backward(d_PE_reward=d_per, d_x=d_x))
    env.stop_tape()
    env.close()
    return out


def tangent(K):
    """K = None: one direction without a K axis."""
    env = _env(T_BACK)
    lead = () if K is None else (K,)
    d_act, d_x0 = _randn(lead + (T_BACK, E, 2 * M), 4), _randn(lead + (E, N), 5)
    out = _time(lambda: env.tangent(d_actions=d_act, d_x0=d_x0))
    env.stop_tape()
    env.close()
    return out


def moments_jvp():
    env = _env(T_BACK)
    env.stop_tape()
    d_x, d_v = _randn((E, N), 6), _randn((E, N), 7)
    out = _time(lambda: env.moments_jvp(d_x=d_x, d_v=d_v))
    if not args.fake:
        torch.cuda.synchronize()
    env.close()
    return out


if __name__ == "__main__":
    print(json.dumps({"what": "grad_python_overhead", "label": args.label, "fake": args.fake, "walk_step": walk_step(),
                      "backward": backward(), "tangent_K1": tangent(None), "tangent_K4": tangent(4), "moments_jvp": moments_jvp()}),
          flush=True)
