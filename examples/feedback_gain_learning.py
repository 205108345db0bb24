"""Closed-loop control learned by gradient descent: the gain G of the feedback law a_t = G m_t (m_t: the Fourier modes
Re E_1..Re E_M, Im E_1..Im E_M of the field each step starts from), optimised with Adam on the gradient of the reference's cost
through the closed loop (env.grad.rollout_feedback -> pic_step_feedback_gain on a tape -> pic_tape_backward_feedback).

    J = sum_t PE_reward_t + lam * sum_t |a_t|^2 L / 4          (the two terms of the reference's Reward, summed over the rollout)

on an ensemble of two-stream environments drawn by the device sampler, each with a gain of its own, starting from the reference's
law G0 = diag(-1 x M, +1 x M) (run_feedback.py:133-135).  Prints J (mean over the ensemble) for each iteration next to the
uncontrolled rollout's and G0's.

    python examples/feedback_gain_learning.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


def run(num_envs=64, N=5000, steps=50, iters=20, N_mesh=250, L=50.0, max_mode=5, lam=0.1, lr=0.02, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    n = 2 * max_mode
    g0 = np.diag(np.concatenate([-np.ones(max_mode), np.ones(max_mode)]))
    # the uncontrolled rollout: zero actions
    env.reset_sampled("two-stream", seed=seed)
    h = env.step_actions_traj(np.zeros((steps, num_envs, n)), history=True)
    J_free = float(h[2].sum(axis=0).mean())
    G = torch.as_tensor(np.broadcast_to(g0, (num_envs, n, n)).copy(), device="cuda").requires_grad_(True)
    opt = torch.optim.Adam([G], lr=lr)
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        env.stop_tape()
        env.reset_sampled("two-stream", seed=seed)          # the same ensemble every iteration
        opt.zero_grad()
        _, _, per, modes = grad.rollout_feedback(env, G, steps)
        a = torch.einsum("eik,tek->tei", G, modes)           # the actions the law took
        J = per.sum(dim=0) + lam * (a ** 2).sum(dim=(0, 2)) * L / 4      # [num_envs]
        J.sum().backward()
        opt.step()
        history.append(float(J.detach().mean()))
        print(f"iter {it:2d}  J = {history[-1]:.6e}  (uncontrolled {J_free:.6e}, G0 {history[0]:.6e})  "
              f"({time.perf_counter() - t0:.3f} s)", flush=True)
    env.stop_tape()
    env.close()
    return J_free, history


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    J_free, h = run(*args)
    print(f"J: uncontrolled {J_free:.6e}, G0 {h[0]:.6e} -> learned {min(h):.6e}")
