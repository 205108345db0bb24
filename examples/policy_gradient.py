"""Closed-loop optimal control with a torch policy trained by backpropagation through the plasma (env.grad.rollout_policy ->
pic_tape_walk_*).  Two policies of the reference's kinds:

  modes: a small MLP on the Fourier modes of the field (the behaviour-cloning / feedback observation)
  state: a DeepSets encoder of the particles, phi(cos q, sin q, p) pooled over particles, then rho (the DDPG / PPO / SAC actor's
         observation)

Each is trained with Adam on the reference's cost, summed over the rollout,

    J = sum_t PE_reward_t + lam * sum_t |a_t|^2 L / 4

on an ensemble of two-stream environments drawn by the device sampler (the same ensemble every iteration).  Prints J (mean over
the ensemble) for each iteration.

    python examples/policy_gradient.py [modes|state|both] [num_envs] [N] [steps] [iterations]
"""
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


class ModesMLP(torch.nn.Module):
    """modes [E, 2 M_o] -> actions [E, 2M]; the last layer starts at zero (a = 0: the uncontrolled plasma)."""

    def __init__(self, obs_modes, max_mode, hidden=64):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(2 * obs_modes, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * max_mode))
        torch.nn.init.zeros_(self.net[-1].weight)
        torch.nn.init.zeros_(self.net[-1].bias)

    def forward(self, m):
        return self.net(m.to(self.net[0].weight.dtype))


class DeepSets(torch.nn.Module):
    """(x, v) [E, N] each -> actions [E, 2M]: phi on (cos q, sin q, v) per particle, q = 2 pi x / L, mean over particles, rho."""

    def __init__(self, L, max_mode, hidden=32):
        super().__init__()
        self.L = L
        self.phi = torch.nn.Sequential(torch.nn.Linear(3, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, hidden), torch.nn.Tanh())
        self.rho = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * max_mode))
        torch.nn.init.zeros_(self.rho[-1].weight)
        torch.nn.init.zeros_(self.rho[-1].bias)

    def forward(self, xv):
        x, v = xv
        dt = self.rho[0].weight.dtype
        q = (2 * math.pi / self.L) * x
        f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1).to(dt)
        return self.rho(self.phi(f).mean(dim=-2))


def make(kind, L, max_mode, obs_modes):
    torch.manual_seed(0)
    return (ModesMLP(obs_modes, max_mode) if kind == "modes" else DeepSets(L, max_mode)).to("cuda")


def iteration(env, policy, kind, steps, obs_modes, lam, L, seed):
    """One forward + backward: returns J [num_envs] (the policy's .grad filled)."""
    env.stop_tape()
    env.reset_sampled("two-stream", seed=seed)
    _, _, per, acts, _ = grad.rollout_policy(env, policy, steps, observe=kind, obs_modes=obs_modes)
    J = per.sum(dim=0) + lam * (acts ** 2).sum(dim=(0, 2)) * L / 4
    J.sum().backward()
    return J.detach()


def run(kind="modes", num_envs=64, N=5000, steps=50, iters=10, N_mesh=250, L=50.0, max_mode=5, obs_modes=8, lam=0.1,
        lr=0.02, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    policy = make(kind, L, max_mode, obs_modes)
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        opt.zero_grad()
        J = iteration(env, policy, kind, steps, obs_modes, lam, L, seed)
        opt.step()
        history.append(float(J.mean()))
        print(f"{kind}  iter {it:2d}  J = {history[-1]:.6e}  ({time.perf_counter() - t0:.3f} s)", flush=True)
    env.stop_tape()
    env.close()
    return history


if __name__ == "__main__":
    kinds = ("modes", "state") if len(sys.argv) < 2 or sys.argv[1] == "both" else (sys.argv[1],)
    args = [int(a) for a in sys.argv[2:]]
    for k in kinds:
        h = run(k, *args)
        print(f"{k}: J {h[0]:.6e} -> {h[-1]:.6e}")
