"""What the rollout recorder costs (profiles/record_cost.md): wall time per step of the same rollout with the recorder off and on,
interleaved A/B on one handle, at config 2 (64 x 1e6, Ng = 256, fp64, streaming) and in the resident regime (256 x 5000).

    python profiles/record_cost.py [--quick] [--json OUT]      # end to end, profiler off
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/record_cost.py --kernels   # kernel times, a run of its own

Each reading is (step K + sync) / K; the medians of `--reps` alternations are reported.  Recorded runs: spectrum rows 0..15, x and
v histograms of 64 bins and a 64 x 64 phase histogram (entropy and KL), as the issue's target specifies."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

REC = dict(modes=16, x_bins=64, v_bins=64, phase_bins=64)


def per_step_ms(env, K, stride):
    if stride:
        env.start_recording(stride=stride, capacity=K, feq=np.full((64, 64), 1e-3), **REC)
    env.sync()
    t0 = time.perf_counter()
    env.step(nsteps=K)
    env.sync()
    ms = (time.perf_counter() - t0) * 1e3 / K
    if stride:
        assert len(env.recorded()) == K // stride
        env.stop_recording()
    return ms


def measure(E_, N, Ng, K, reps, strides):
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E_, N, Ng, dt=0.1)
    env.reset_sampled(seed=1)
    env.step(nsteps=10)
    env.sync()
    out = {s: [] for s in (0,) + tuple(strides)}
    for _ in range(reps):
        for s in out:
            out[s].append(per_step_ms(env, K, s))
    res = {"envs": E_, "N": N, "Ng": Ng, "schedule": env._h.schedule(), "K": K, "reps": reps}
    base = statistics.median(out[0])
    res["off_ms_per_step"] = base
    res["off_spread"] = [min(out[0]), max(out[0])]
    for s in strides:
        m = statistics.median(out[s])
        res[f"stride{s}_ms_per_step"] = m
        res[f"stride{s}_spread"] = [min(out[s]), max(out[s])]
        res[f"stride{s}_overhead_pct"] = 100.0 * (m / base - 1)
        res[f"stride{s}_us_per_record"] = 1e3 * (m - base) * s
    if N >= 100000:
        gbs = env.stream_probe(10)
        res["stream_probe_GBps"] = gbs
        res["read_x_v_us_at_probe_rate"] = E_ * N * 16 / (gbs * 1e9) * 1e6
    env.close()
    return res


def kernels_only():
    """A run for rocprofv3: recorded steps at both sizes (the kernel statistics carry record_hist_kernel / record_finish_kernel)."""
    from ocplasma_amd.env.batched import BatchedPIC
    for E_, N, K in ((64, 1_000_000, 20), (256, 5000, 50)):
        env = BatchedPIC(E_, N, 256, dt=0.1)
        env.reset_sampled(seed=1)
        env.start_recording(stride=1, capacity=K, feq=np.full((64, 64), 1e-3), **REC)
        env.step(nsteps=K)
        env.sync()
        env.stop_recording()
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kernels:
        kernels_only()
        return
    reps = 2 if a.quick else a.reps
    rows = [measure(64, 1_000_000, 256, 40, reps, (10, 1)), measure(256, 5000, 256, 200, reps, (1, 10))]
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
