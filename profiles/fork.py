"""What a copy of environments costs (profiles/fork.md): pic_copy_envs between two handles -- identity and a broadcast of one
environment to all -- as kernel time and wall time per call, the next step() behind it, the handle's stream_probe() rate, and the
route there was before: indexed copy_ through torch_views() followed by refresh().  The two routes are timed interleaved on one
box, `--rounds` rounds, at config 2's shape (64 x 1e6 float64) and the reference's (256 x 5000).

    python profiles/fork.py [--rounds 3] [--out profiles/fork.md] [--write-through]

The numbers replace what stands between the two marker lines of --out for this build (BEGIN / END below); the rest of the file,
written by hand, is kept.  --write-through measures a build of the library whose copy_rows_kernel stores write-through instead of
plainly (-DPIC_COPY_WRITE_THROUGH=1, compiled into profiles/bin/ on first use and loaded instead of the package's library),
so that the step behind the copy can be compared between the two store policies.  The choices inside copy_rows_kernel are also
measured on bare buffers by profiles/fork_probe.hip."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e6


def measure(E_, N, Ng, rounds, reps):
    import torch
    from ocplasma_amd.env.batched import BatchedPIC
    a, b = BatchedPIC(E_, N, Ng, dt=0.1), BatchedPIC(E_, N, Ng, dt=0.1)
    for h in (a, b):
        h.reset_sampled(seed=1)
        h.step(nsteps=2)
        h.sync()
    ta, tb = a.torch_views(), b.torch_views()
    ident = torch.arange(E_, device="cuda")
    zeros = torch.zeros(E_, dtype=torch.int64, device="cuda")

    def both():
        b.sync()
        torch.cuda.synchronize()

    def old(index):
        for k in ("x", "v"):
            tb[k].copy_(ta[k][index])
        torch.cuda.synchronize()
        b.refresh()

    out = {k: [] for k in ("new_identity", "new_broadcast", "new_next_step", "old_identity", "old_broadcast", "old_next_step",
                           "plain_step", "kernel_identity", "kernel_broadcast")}
    for _ in range(rounds):
        for _ in range(reps):
            out["new_identity"].append(timed(lambda: b.copy_from(a), both))
            out["old_identity"].append(timed(lambda: old(ident), both))
            out["new_broadcast"].append(timed(lambda: b.copy_from(a, 0), both))
            out["new_next_step"].append(timed(lambda: b.step(), both))
            out["old_broadcast"].append(timed(lambda: old(zeros), both))
            out["old_next_step"].append(timed(lambda: b.step(), both))
            out["plain_step"].append(timed(lambda: b.step(), both))
        b.profile(True)
        for _ in range(reps):
            b.copy_from(a)
        ms, n = b.profile_read()["sweep_aux"]
        out["kernel_identity"].append(ms / n * 1e3)
        b.profile(True)
        for _ in range(reps):
            b.copy_from(a, 0)
        ms, n = b.profile_read()["sweep_aux"]
        out["kernel_broadcast"].append(ms / n * 1e3)
        b.profile(False)
    gbs = b.stream_probe(10)
    moved = 4.0 * E_ * a._h.device_ptrs()["ld"] * 8
    res = {"envs": E_, "N": N, "Ng": Ng, "schedule": b._h.schedule(), "stream_probe_GBps": gbs,
           "identity_us_at_probe_rate": moved / (gbs * 1e9) * 1e6}
    for k, v in out.items():
        res[k] = (statistics.median(v), min(v), max(v))
    a.close()
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "fork.md"))
    ap.add_argument("--write-through", action="store_true")
    a = ap.parse_args()
    tag = "write-through stores" if a.write_through else "plain stores"
    if a.write_through:
        from ocplasma_amd import _build
        variant = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bin", "libpicstep_write_through.so")
        if not os.path.exists(variant):
            os.makedirs(os.path.dirname(variant), exist_ok=True)
            _build._compile(variant, ("PIC_COPY_WRITE_THROUGH=1",))
        _build.LIB = variant
    begin, end = f"<!-- BEGIN profiles/fork.py: {tag} -->", f"<!-- END profiles/fork.py: {tag} -->"
    lines = [begin, f"## Measured by profiles/fork.py ({tag})", "",
             "Microseconds per call: median (min .. max) over rounds x reps; wall = call + synchronisation; kernel = the two copy",
             "kernels of one call between HIP events.", ""]
    for E_, N in ((64, 1_000_000), (256, 5000)):
        r = measure(E_, N, 256, a.rounds, a.reps)
        lines += [f"### {E_} x {N} float64, Ng = 256 ({r['schedule']}); stream_probe {r['stream_probe_GBps']:.0f} GB/s: "
                  f"x and v of all environments read and written once in {r['identity_us_at_probe_rate']:.1f} us", "",
                  "| what | us |", "|---|---|"]
        for k in ("kernel_identity", "kernel_broadcast", "new_identity", "old_identity", "new_broadcast", "old_broadcast",
                  "new_next_step", "old_next_step", "plain_step"):
            m, lo, hi = r[k]
            lines.append(f"| {k} | {m:.1f} ({lo:.1f} .. {hi:.1f}) |")
        lines.append("")
        print("\n".join(lines[-14:]), flush=True)
    lines.append(end)
    block = "\n".join(lines) + "\n"
    old = open(a.out).read() if os.path.exists(a.out) else ""
    if begin in old and end in old:
        new = old[:old.index(begin)] + block + old[old.index(end) + len(end) + 1:]
    else:
        new = old + ("\n" if old else "") + block
    with open(a.out, "w") as f:
        f.write(new)


if __name__ == "__main__":
    main()
