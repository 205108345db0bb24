"""A policy that observes the fluid moments of the plasma (env.grad.rollout_policy(observe="moments")).

At every step the policy sees o_t [num_envs, 3, N_mesh], the density, momentum density and twice the kinetic-energy density on
the mesh, derives (n, u, T) from it in torch, pools each over 8 nodes and maps the result linearly (then tanh) to the actuator's
coefficients.  It is trained with Adam on

    J = sum_t PE_reward_t + lam * sum_t |a_t|^2 L / 4

through the plasma: the backward walks the tape and hands the policy's cotangent on o_t to pic_tape_moments_cot.  Prints J
(mean over the ensemble) for each iteration; it goes down.

    python examples/moments_observation.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


class PooledFluid(torch.nn.Module):
    """moments [E, 3, Ng] -> actions [E, 2M]: (n - n0, u, T) averaged over `width` nodes, one linear layer, tanh.  The layer
    starts small, so the first rollout is almost the uncontrolled plasma."""

    def __init__(self, N_mesh, max_mode, n0=1.0, width=8, amplitude=0.5):
        super().__init__()
        self.n0, self.width, self.amplitude = n0, width, amplitude
        self.lin = torch.nn.Linear(3 * (N_mesh // width), 2 * max_mode, dtype=torch.float64)
        torch.nn.init.normal_(self.lin.weight, std=1e-3)
        torch.nn.init.zeros_(self.lin.bias)

    def forward(self, o):
        m0, m1, m2 = o[:, 0], o[:, 1], o[:, 2]
        n = m0.clamp_min(1e-12)
        u = m1 / n
        T = m2 / n - u * u
        f = torch.stack([m0 - self.n0, u, T - T.mean(dim=1, keepdim=True)], dim=1)    # [E, 3, Ng]
        f = f.reshape(f.shape[0], 3, -1, self.width).mean(-1).flatten(1)
        return self.amplitude * torch.tanh(self.lin(f))


def run(num_envs=16, N=5000, steps=30, iters=8, N_mesh=248, L=50.0, max_mode=3, lam=0.1, lr=1e-3, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    torch.manual_seed(0)
    policy = PooledFluid(N_mesh, max_mode).to("cuda")
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    history = []
    for it in range(iters):
        env.stop_tape()
        env.reset_sampled("two-stream", seed=seed)
        opt.zero_grad()
        _, _, per, acts, _ = grad.rollout_policy(env, policy, steps, observe="moments")
        J = per.sum(dim=0) + lam * (acts ** 2).sum(dim=(0, 2)) * L / 4
        J.sum().backward()
        opt.step()
        history.append(float(J.detach().mean()))
        print(f"iter {it:2d}  J = {history[-1]:.6e}", flush=True)
    env.stop_tape()
    n, u, T = env.fluid()
    print(f"final state: n in [{n.min():.3f}, {n.max():.3f}]  u in [{u.min():.3f}, {u.max():.3f}]  T in [{T.min():.3f}, {T.max():.3f}]")
    env.close()
    return history


if __name__ == "__main__":
    h = run(*[int(a) for a in sys.argv[1:]])
    print(f"J {h[0]:.6e} -> {h[-1]:.6e}")
