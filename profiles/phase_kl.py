"""What the smoothed phase-space KL costs (profiles/phase_kl.md): the kernels of kl_smooth (deposit + finish) and kl_smooth_grad
(deposit + finish + gather) on one shape per run.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/phase_kl.py E N BINS     # kernel times, a run of its own
    python profiles/phase_kl.py E N BINS --probe                                                # + the time to read x, v once

Config 2's shape is 64 1000000, the reference shape 64 5000; BINS 64 or 250.  Each run makes 4 calls of each entry (the first
a warm-up)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def main():
    from ocplasma_amd.env.batched import BatchedPIC
    E, N, nb = (int(a) for a in sys.argv[1:4])
    env = BatchedPIC(E, N, 256, dt=0.1)
    env.reset_sampled("bump-on-tail", seed=1)
    feq = env.phase_density_smooth(nb, -25.0, 25.0).mean(axis=0)      # the initial state's density as the target
    env.step(nsteps=2)
    for _ in range(4):
        kl = env.kl_smooth(feq, -25.0, 25.0)
        gx, gv = env.kl_smooth_grad(feq, None, -25.0, 25.0)
    print(f"E={E} N={N} bins={nb}: kl[0]={kl[0]:.6e} |g_x|max={np.abs(gx).max():.3e} |g_v|max={np.abs(gv).max():.3e}")
    if "--probe" in sys.argv:
        gbs = env.stream_probe(10)
        print(f"stream probe {gbs:.0f} GB/s: reading x, v once takes {E * N * 16 / (gbs * 1e9) * 1e6:.1f} us")
    env.close()


if __name__ == "__main__":
    main()
