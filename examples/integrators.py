"""What the cheaper integrators cost in physics: one two-stream initial state stepped under every scheme of PIC's `integrator=`
option (the reference's symplectic_4th_order, symplectic_euler, verlet, forward_euler).  Per scheme: the relative drift of the
total energy, the growth rate of the field energy over the linear phase (interpret.landau.damping_rate on a recording) and the
wall time per step.

    python examples/integrators.py [num_envs] [N] [steps]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, TwoStream  # noqa: E402
from ocplasma_amd.interpret import landau  # noqa: E402

SCHEMES = ("symplectic_4th_order", "symplectic_euler", "verlet", "forward_euler")


def run(num_envs=4, N=20000, steps=300, N_mesh=128, L=50.0, dt=0.1, seed=11, t_linear=(2.0, 12.0)):
    np.random.seed(seed)
    dist = TwoStream(v0=3.0, sigma=1.0, n_samples=N, L=L)
    xs, vs = [], []
    for _ in range(num_envs):
        dist.reinit()
        x, v = dist.get_sample()
        xs.append(x)
        vs.append(v * (1 + 0.1 * np.sin(2 * np.pi * 2 * x / L)))     # PIC.initialize perturbation, n_mode = 2
    out = {}
    for scheme in SCHEMES:
        env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=dt, integrator=scheme)
        env.reset(np.stack(xs), np.stack(vs))
        ke0, pe0, _ = env.energies()
        env.step(None, 5)                                              # warm-up of the kernels, then the same start again
        env.reset(np.stack(xs), np.stack(vs))
        env.sync()
        with env.recording(stride=1, capacity=steps + 1) as session:
            env.record_now()
            t0 = time.perf_counter()
            ke, pe, _ = env.step_history(None, steps)
            ms = (time.perf_counter() - t0) * 1e3 / steps
        H0, H = ke0 + pe0, ke + pe
        drift = np.max(np.abs(H - H0) / np.abs(H0), axis=0)
        gamma = landau.damping_rate(session.record, *t_linear)
        env.close()
        out[scheme] = dict(drift=drift, gamma=gamma, ms=ms)
        print(f"{scheme:22s} max |H - H0| / H0 = {np.max(drift):.3e}   growth rate on t in {t_linear} = "
              f"{np.mean(gamma):+.4f} (+- {np.std(gamma):.1e})   {ms:.3f} ms per step (with the energy history)")
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    run(**{k: int(v) for k, v in zip(("num_envs", "N", "steps"), args[:3])})
