"""Open-loop control on the reference's whole cost: gradient descent on the actions of a small rollout with

    J = sum_t ( r_kl_t + r_pe_t + r_ie_t )          (Reward.compute_cost: the KL of the phase-space density against the initial
                                                     one, the electric energy, the input energy |a_t|^2 L / 4)

where r_kl is the smoothed KL of DESIGN.md 7g, recorded after every step on the tape and differentiated with the energies
(env.grad.rollout(..., kl=...)).  The target feq is the smoothed density of the initial state.  Prints the cost
and its three parts (mean over the ensemble) for each iteration.

    python examples/kl_control.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


def run(num_envs=8, N=5000, steps=20, iters=10, N_mesh=250, L=50.0, max_mode=3, bins=32, vmin=-8.0, vmax=8.0, lr=0.05, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.reset_sampled("two-stream", seed=seed)
    feq = env.phase_density_smooth(bins, vmin, vmax)         # [num_envs, bins, bins]: every environment against its own start
    kl = dict(feq=feq, vmin=vmin, vmax=vmax)
    a = torch.zeros((steps, num_envs, 2 * max_mode), dtype=torch.float64, device="cuda", requires_grad=True)
    history = []
    for it in range(iters):
        env.stop_tape()
        env.reset_sampled("two-stream", seed=seed)           # the same ensemble every iteration
        _, _, r_pe, r_kl = grad.rollout(env, a, kl=kl)
        r_ie = (a ** 2).sum(dim=2) * L / 4
        J = (r_kl + r_pe + r_ie).sum(dim=0)                  # [num_envs]
        (g,) = torch.autograd.grad(J.sum(), a)
        with torch.no_grad():
            a -= lr * g
        history.append(float(J.detach().mean()))
        print(f"iter {it:2d}  cost = {history[-1]:.6e}  (kl {float(r_kl.sum(0).mean()):.4e}  pe {float(r_pe.sum(0).mean()):.4e}"
              f"  ie {float(r_ie.sum(0).mean()):.4e})", flush=True)
    env.stop_tape()
    env.close()
    return history


if __name__ == "__main__":
    h = run(*[int(x) for x in sys.argv[1:]])
    print(f"cost: {h[0]:.6e} -> {h[-1]:.6e}")
