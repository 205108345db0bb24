"""Cost of a closed loop under an MLP policy: wall time per step, host clock around work that ends in a device
synchronise, of

  a  step_policy: the policy and the steps in one call
  b  the Python loop modes_torch -> float64 torch module -> step_actions_torch on a stream shared with torch (no host wait)
  c  step_actions_traj with precomputed actions: the steps with no policy at all (runs on a checkout without the policy too)
  d  step_feedback_gain in one call: a law that lives inside the kernels
  k  pic_policy_eval alone, back to back on the device: one launch of the policy kernel per call

under a [6, 64, 64, 6] tanh policy (M = M_o = 3) at 256 x 5000 (Ng 250), 1024 x 5000 and config 2's shape (64 x 1e6, Ng 256).
A timed window is a few calls of T steps each, back to back.  The variants alternate within every round; per variant the median, the fastest and the slowest round are reported, in
microseconds per step.  One JSON line per shape.

    python profiles/policy_rollout.py [--shape ref|wide|cfg2|all] [--variants abcdk] [--rounds 7]
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

SHAPES = {"ref": (256, 5000, 250, 100, 10), "wide": (1024, 5000, 250, 100, 5), "cfg2": (64, 1_000_000, 256, 20, 2)}   # E, N, Ng, T, calls per timed window
M = 3
WIDTHS = [2 * M, 64, 64, 2 * M]


def measure(E, N, Ng, T, calls, variants, rounds):
    import torch
    env = BatchedPIC(E, N, Ng, L=50.0, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(E_field(50.0, Ng, M))
    env.use_torch_stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0)
    runs = {}
    if set(variants) & set("abk"):
        from ocplasma_amd.control.policy import MLPPolicy, param_count
        pol = MLPPolicy(WIDTHS, "tanh", torch.tensor(0.1 * rng.standard_normal(param_count(WIDTHS)), **f64), M,
                        obs_scale=torch.full((2 * M,), 8.0, **f64))
        net = pol.to_torch().to("cuda")

        def run_a():
            env.step_policy(pol, T, history=False, on_device=True)

        def run_b():
            with torch.no_grad():
                for _ in range(T):
                    env.step_actions_torch(pol.torch_actions(net, env.modes_torch(M)).contiguous())

        from ocplasma_amd.env._arrays import Mem
        mem = Mem.of(env, force_device=True)
        spec, keep = pol.spec(mem, E)
        outs = [torch.empty((E, 2 * M), **f64) for _ in range(3)]

        def run_k():
            for _ in range(T):
                env._h.policy_eval(spec, 0, 0, 0, mem.kind, *(o.data_ptr() for o in outs))
        runs.update(a=run_a, b=run_b, k=run_k)
    acts = torch.tensor(rng.uniform(-0.5, 0.5, (T, E, 2 * M)), **f64)
    g0 = np.diag(np.concatenate([-np.ones(M), np.ones(M)]))
    G = torch.tensor(g0 + 0.05 * rng.standard_normal((E, 2 * M, 2 * M)), **f64)
    runs["c"] = lambda: env.step_actions_traj_torch(acts)
    runs["d"] = lambda: env.step_feedback_gain(G, T)
    order = [v for v in variants if v in runs]
    times = {v: [] for v in order}
    for v in order:                      # warm-up: code objects, torch's kernels, the handle's buffers
        runs[v]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in order:                  # interleaved: drift and neighbours hit every variant alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                runs[v]()
            torch.cuda.synchronize()
            times[v].append(1e6 * (time.perf_counter() - t0) / (T * calls))
    out = {"E": E, "N": N, "Ng": Ng, "T": T, "calls_per_window": calls, "rounds": rounds, "schedule": env._h.schedule(), "bad": env.bad_count()}
    for v in order:
        t = sorted(times[v])
        out[v] = {"median_us": round(t[len(t) // 2], 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2)}
    med = lambda v: out[v]["median_us"]
    if "a" in out and "b" in out:
        out["a_over_b"] = round(med("a") / med("b"), 3)
    if "a" in out and "c" in out:
        out["a_minus_c_us"] = round(med("a") - med("c"), 2)
    if "a" in out and "d" in out:
        out["a_minus_d_us"] = round(med("a") - med("d"), 2)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["ref", "wide", "cfg2", "all"])
    ap.add_argument("--variants", default="abcdk")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    for name in (("ref", "wide", "cfg2") if args.shape == "all" else (args.shape,)):
        print(json.dumps({"shape": name, **measure(*SHAPES[name], args.variants, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
