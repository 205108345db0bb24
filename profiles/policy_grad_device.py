"""Cost of one training iteration through an MLP policy: wall time of forward plus backward, host clock around
work that ends in a device synchronise, of

  a  env.grad.rollout_mlp: start_tape + tape_step_policy, then one backward_policy (the policy's VJP kernel inside the walk)
  b  env.grad.rollout_policy under the policy's float64 torch twin: back to Python every step in both directions (the yardstick)
  c  an open-loop tape of the same length (step_actions_traj) and pic_tape_backward: the floor, no policy at all
  k  pic_policy_vjp without g_params, back to back on the device: one launch of policy_vjp_kernel per call
  r  pic_policy_vjp with g_params: the kernel, the reduction over environments and the copy of [P] per call

under a [6, 64, 64, 6] tanh policy (M = M_o = 3) at 256 x 5000 (Ng 250, T = 100) and config 2's shape (64 x 1e6, Ng 256, T = 20).
The variants alternate within every round; per variant the median, the fastest and the slowest round are reported: a, b, c in
milliseconds per iteration, k and r in microseconds per call.  One JSON line per shape.

    python profiles/policy_grad_device.py [--shape ref|cfg2|all] [--variants abckr] [--rounds 7]
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

SHAPES = {"ref": (256, 5000, 250, 100), "cfg2": (64, 1_000_000, 256, 20)}   # E, N, Ng, T
M = 3
WIDTHS = [2 * M, 64, 64, 2 * M]
LAM, L = 0.1, 50.0


def measure(E, N, Ng, T, variants, rounds):
    import torch
    from ocplasma_amd.control.policy import MLPPolicy, param_count
    from ocplasma_amd.env import grad
    from ocplasma_amd.env._arrays import Mem
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.set_actuator(E_field(L, Ng, M))
    env.use_torch_stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(0)
    pol = MLPPolicy(WIDTHS, "tanh", torch.tensor(0.1 * rng.standard_normal(param_count(WIDTHS)), **f64), M,
                    obs_scale=torch.full((2 * M,), 8.0, **f64))
    net = pol.to_torch().to("cuda")
    acts0 = torch.tensor(rng.uniform(-0.5, 0.5, (T, E, 2 * M)), **f64)

    def cost(per, acts):
        return (per.sum(dim=0) + LAM * (acts ** 2).sum(dim=(0, 2)) * L / 4).sum()

    def fresh():
        env.stop_tape()
        env.reset_sampled("two-stream", seed=1)

    def run_a():
        fresh()
        params = pol.params.clone().requires_grad_(True)
        out = grad.rollout_mlp(env, pol, params, T)
        cost(out[2], out[3]).backward()

    def run_b():
        fresh()
        net.zero_grad()
        out = grad.rollout_policy(env, lambda o: pol.torch_actions(net, o), T, observe="modes", obs_modes=M)
        cost(out[2], out[3]).backward()

    def run_c():
        fresh()
        a = acts0.clone().requires_grad_(True)
        out = grad.rollout(env, a)
        cost(out[2], a).backward()

    mem = Mem.of(env, force_device=True)
    spec, keep = pol.spec(mem, E)
    obs, pre, cot = (torch.tensor(rng.standard_normal((E, n)), **f64) for n in (2 * M, 2 * M, 2 * M))
    gp, go, gu = torch.empty(pol.n_params, **f64), torch.empty((E, 2 * M), **f64), torch.empty((E, 2 * M), **f64)

    def run_k():
        for _ in range(T):
            env._h.policy_vjp(spec, obs.data_ptr(), pre.data_ptr(), cot.data_ptr(), mem.kind, 0, go.data_ptr(), gu.data_ptr())

    def run_r():
        for _ in range(T):
            env._h.policy_vjp(spec, obs.data_ptr(), pre.data_ptr(), cot.data_ptr(), mem.kind, gp.data_ptr(), go.data_ptr(), gu.data_ptr())

    runs = {"a": run_a, "b": run_b, "c": run_c, "k": run_k, "r": run_r}
    order = [v for v in variants if v in runs]
    times = {v: [] for v in order}
    for v in order:                      # warm-up: code objects, torch's kernels, the handle's buffers
        runs[v]()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v in order:                  # interleaved: drift and neighbours hit every variant alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runs[v]()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            times[v].append(1e6 * dt / T if v in "kr" else 1e3 * dt)
    env.stop_tape()
    out = {"E": E, "N": N, "Ng": Ng, "T": T, "rounds": rounds, "schedule": env._h.schedule(), "bad": env.bad_count(),
           "units": {"a": "ms", "b": "ms", "c": "ms", "k": "us per call", "r": "us per call"}}
    for v in order:
        t = sorted(times[v])
        out[v] = {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3), "max": round(t[-1], 3)}
    med = lambda v: out[v]["median"]  # noqa: E731
    if "a" in out and "b" in out:
        out["a_over_b"] = round(med("a") / med("b"), 3)
    if "a" in out and "c" in out:
        out["a_minus_c_us_per_step"] = round(1e3 * (med("a") - med("c")) / T, 2)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["ref", "cfg2", "all"])
    ap.add_argument("--variants", default="abckr")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    for name in (("ref", "cfg2") if args.shape == "all" else (args.shape,)):
        print(json.dumps({"shape": name, **measure(*SHAPES[name], args.variants, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
