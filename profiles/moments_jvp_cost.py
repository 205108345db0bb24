"""What the moments' tangents cost on a tape (profiles/moments_jvp.md): `tangent(moments=True)` against plain `tangent()` on the
same tape, interleaved, best of 3, for K = 1 and K = 4 directions, on one shape per run.

    python profiles/moments_jvp_cost.py E N NG T                                               # wall times
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/moments_jvp_cost.py E N NG T --once    # kernel times

Config 2's shape is 64 1000000 256 20, the reference shape 64 5000 250 100.  Everything stays in device memory."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    E, N, Ng, T = (int(a) for a in sys.argv[1:5])
    once = "--once" in sys.argv
    M = 3
    env = BatchedPIC(E, N, Ng, dt=0.1)
    env.set_actuator(oc.E_field(env.L, Ng, M))
    env.reset_sampled("bump-on-tail", seed=1)
    gen = torch.Generator(device="cuda").manual_seed(1)
    a = 0.5 * torch.rand((T, E, 2 * M), dtype=torch.float64, device="cuda", generator=gen) - 0.25
    env.start_tape(T)
    env.step_actions_traj_torch(a)
    for K in (1, 4):
        du = torch.randn((K, T, E, 2 * M), dtype=torch.float64, device="cuda", generator=gen)
        best = {False: float("inf"), True: float("inf")}
        for rep in range(1 if once else 4):                # (the first repetition warms up and reserves the working memory)
            for mom in (False, True):
                env.sync()
                t0 = time.perf_counter()
                out = env.tangent(d_actions=du, moments=mom)
                env.sync()
                if rep or once:
                    best[mom] = min(best[mom], time.perf_counter() - t0)
        st = env.tape_stats()
        extra = (best[True] - best[False]) / T
        print(f"E={E} N={N} Ng={Ng} T={T} K={K}: tangent {best[False] * 1e3:.2f} ms, with moments {best[True] * 1e3:.2f} ms, "
              f"+{extra * 1e6:.1f} us per step; launches {st['launches']}, |dm|max {float(out['moments'].abs().max()):.3e}")
    env.stop_tape()
    env.close()


if __name__ == "__main__":
    main()
