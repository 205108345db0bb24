"""What the fluid moments cost (profiles/moments.md): the kernels of `moments` (max + deposit + finish) and `moments_vjp`, next
to the smoothed KL's deposit at 64 x 64 bins on the same device, on one shape per run.

    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/moments.py E N NG     # kernel times, a run of its own
    python profiles/moments.py E N NG --probe                                               # + the time to read x, v once

Config 2's shape is 64 1000000 256, the reference shape 64 5000 250.  Each run makes 4 calls of each entry (the first a
warm-up), all in device memory."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from ocplasma_amd.env.batched import BatchedPIC
    E, N, Ng = (int(a) for a in sys.argv[1:4])
    env = BatchedPIC(E, N, Ng, dt=0.1)
    env.reset_sampled("bump-on-tail", seed=1)
    feq = env.phase_density_smooth(64, -25.0, 25.0).mean(axis=0)
    env.step(nsteps=2)
    g = torch.randn((E, 3, Ng), dtype=torch.float64, device="cuda")
    for _ in range(4):
        m = env.moments_torch()
        gx, gv = env.moments_vjp(g)
        kl = env.kl_smooth(feq, -25.0, 25.0)
    n = env.fields()[0]
    print(f"E={E} N={N} Ng={Ng}: m0 == n: {bool(np.array_equal(m[:, 0].cpu().numpy(), n))} sum m0 / Ng = {float(m[0, 0].sum()) / Ng:.15f} "
          f"|g_x|max={float(gx.abs().max()):.3e} |g_v|max={float(gv.abs().max()):.3e} kl[0]={kl[0]:.6e}")
    if "--probe" in sys.argv:
        gbs = env.stream_probe(10)
        print(f"stream probe {gbs:.0f} GB/s: reading x, v once takes {E * N * 16 / (gbs * 1e9) * 1e6:.1f} us")
    env.close()


if __name__ == "__main__":
    main()
