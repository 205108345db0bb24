"""What a step costs under each integrator (profiles/integrators.md): wall time per step, profiler off, at

  cfg2      config 2: 64 x 1e6, Ng 256, fp64, bump-on-tail, streaming -- one step per call and 20 steps per call
  resident  256 x N = 5000, Ng 250, fp64, two-stream, the resident schedule, 20 steps per call
  cfg3      config 3's shape: 128 x 1e6, Ng 512, float32 with fixed-point positions, two-stream, 20 steps per call

    python profiles/integrators.py [--quick] [--json OUT]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/integrators.py --kernels    # a run of its own

Each reading is (K steps in calls of `per_call` + sync) / K; schemes are interleaved, the median of `--reps` rounds reported."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCHEMES = ("symplectic_4th_order", "symplectic_euler", "verlet", "forward_euler")
SHAPES = {
    "cfg2": dict(E=64, N=1_000_000, Ng=256, dtype="float64", pos=None, kind="bump-on-tail"),
    "resident": dict(E=256, N=5000, Ng=250, dtype="float64", pos=None, kind="two-stream"),
    "cfg3": dict(E=128, N=1_000_000, Ng=512, dtype="float32", pos="fixed32", kind="two-stream"),
}


def per_step_ms(env, K, per_call):
    env.sync()
    t0 = time.perf_counter()
    for _ in range(K // per_call):
        env.step(None, per_call)
    env.sync()
    return (time.perf_counter() - t0) * 1e3 / K


def measure(shape, per_call, K, reps):
    from ocplasma_amd.env.batched import BatchedPIC
    s = SHAPES[shape]
    env = BatchedPIC(s["E"], s["N"], s["Ng"], dt=0.1, dtype=s["dtype"], position_dtype=s["pos"])
    env.reset_sampled(s["kind"], seed=1)
    sched = env._h.schedule()
    times = {k: [] for k in SCHEMES}
    for scheme in SCHEMES:                    # warm-up of every kernel
        env._h.set_integrator(scheme)
        per_step_ms(env, per_call * 2, per_call)
    for _ in range(reps):
        for scheme in SCHEMES:
            env._h.set_integrator(scheme)
            env.step(None, 1)                 # (the first step after a switch deposits x once)
            times[scheme].append(per_step_ms(env, K, per_call))
    env.close() if hasattr(env, "close") else None
    return sched, {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="config 2, 20 steps per call, each scheme once (for rocprofv3)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.kernels:
        from ocplasma_amd.env.batched import BatchedPIC
        s = SHAPES["cfg2"]
        env = BatchedPIC(s["E"], s["N"], s["Ng"], dt=0.1)
        env.reset_sampled(s["kind"], seed=1)
        for scheme in SCHEMES:
            env._h.set_integrator(scheme)
            env.step(None, 20)
            env.sync()
        return
    reps = 2 if args.quick else args.reps
    out = {}
    for shape, per_call, K in (("cfg2", 1, 20), ("cfg2", 20, 40), ("resident", 20, 100), ("cfg3", 20, 40)):
        sched, ms = measure(shape, per_call, K, reps)
        key = f"{shape}_per_call{per_call}"
        out[key] = {"schedule": sched, "ms_per_step": ms}
        print(key, sched, json.dumps({k: round(v, 4) for k, v in ms.items()}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
