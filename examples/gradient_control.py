"""Open-loop optimal control by gradient descent: the actuator coefficients of every step of a rollout, optimised with Adam on
the gradient of the reference's cost through the particle dynamics (env.grad.rollout -> pic_tape_backward).

    J = sum_t PE_reward_t + lam * sum_t |a_t|^2 L / 4          (the two terms of the reference's Reward, summed over the rollout)

on an ensemble of two-stream environments drawn by the device sampler.  Prints J (mean over the ensemble) for each iteration.

    python examples/gradient_control.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


def run(num_envs=64, N=5000, steps=50, iters=20, N_mesh=250, L=50.0, max_mode=5, lam=0.1, lr=0.05, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    a = torch.zeros((steps, num_envs, 2 * max_mode), dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([a], lr=lr)
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        env.stop_tape()
        env.reset_sampled("two-stream", seed=seed)          # the same ensemble every iteration
        opt.zero_grad()
        _, _, per = grad.rollout(env, a)
        J = per.sum(dim=0) + lam * (a ** 2).sum(dim=(0, 2)) * L / 4      # [num_envs]
        J.sum().backward()
        opt.step()
        history.append(float(J.detach().mean()))
        print(f"iter {it:2d}  J = {history[-1]:.6e}  ({time.perf_counter() - t0:.3f} s)", flush=True)
    env.stop_tape()
    env.close()
    return history


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    h = run(*args)
    print(f"J: {h[0]:.6e} -> {h[-1]:.6e}")
