"""Sampling-based model-predictive control (MPPI) of the two-stream instability on copies of the plant.

Every round the planner clones the plant's present state into `samples` environments on the device
(`BatchedPIC.copy_from`), rolls out that many perturbed action sequences in one call, weights them by the field energy
they lead to and applies the first action of the weighted mean to the plant (`env.plan.MPPI`).  A clone continues bit for
bit like the plant, so the rollout of the unperturbed sequence is exactly what the plant does next.  The shape is the
reference's feedback run: N = 5000 particles, 250 cells, the first modes of the actuator.

    python examples/mppi_control.py [steps] [samples] [horizon]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd
from ocplasma_amd import BatchedPIC, E_field
from ocplasma_amd.env.plan import MPPI


def run(steps=150, samples=64, horizon=10, N=5000, N_mesh=250, L=50.0, max_mode=3, sigma=0.05, temperature=0.002, beta=1e-3,
        seed=11, verbose=True):
    free = BatchedPIC(1, N, N_mesh, L=L, dt=0.1)
    plant = BatchedPIC(1, N, N_mesh, L=L, dt=0.1)
    plant.set_actuator(E_field(L, N_mesh, max_mode))
    for env in (free, plant):
        env.reset_sampled("two-stream", v0=3.0, sigma=1.0, A=0.1, n_mode=2, seed=seed)
    planner = MPPI(plant, samples=samples, horizon=horizon, sigma=sigma, temperature=temperature, beta=beta, seed=seed)
    pe_free = free.step_history(None, steps)[2][:, 0]
    pe_ctrl, effort = [], []
    for k in range(steps):
        planner.plan()
        a = planner.act()
        pe_ctrl.append(plant.energies()[2][0])
        effort.append(np.abs(a).max())
        if verbose and k % 10 == 0:
            print(f"step {k:4d}  field energy: free {pe_free[k]:.4e}  MPPI {pe_ctrl[-1]:.4e}  max|action| {effort[-1]:.3f}")
    planner.close()
    free.close()
    plant.close()
    return pe_free, np.array(pe_ctrl), np.array(effort)


if __name__ == "__main__":
    pf, pc, eff = run(*[int(v) for v in sys.argv[1:]])
    print(f"peak field energy: free {pf.max():.4e}, MPPI {pc.max():.4e} (ratio {pc.max() / pf.max():.3f}); "
          f"mean over the last quarter: free {pf[-len(pf) // 4:].mean():.4e}, MPPI {pc[-len(pc) // 4:].mean():.4e}")
