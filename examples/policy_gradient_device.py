"""The "modes" loop of examples/policy_gradient.py with the policy on the device in both directions (env.grad.rollout_mlp ->
pic_tape_step_policy / pic_tape_backward_policy): one forward call and one backward call per iteration, no step
returns to Python.  An MLP on the Fourier modes of the field is trained with Adam on the reference's cost, summed over the rollout,

    J = sum_t PE_reward_t + lam * sum_t |a_t|^2 L / 4

on an ensemble of two-stream environments drawn by the device sampler (the same ensemble every iteration).  The optimiser works
on the float64 torch twin of the packed policy (MLPPolicy.to_torch); `unpack_grad` gives the device's flat gradient the layers'
shapes.  Prints J (mean over the ensemble) for each iteration.

    python examples/policy_gradient_device.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.control.policy import MLPPolicy  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


def make(max_mode, obs_modes, hidden=64):
    """modes [E, 2 M_o] -> actions [E, 2M]; the last layer starts at zero (a = 0: the uncontrolled plasma)."""
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(2 * obs_modes, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * max_mode)).double()
    torch.nn.init.zeros_(net[-1].weight)
    torch.nn.init.zeros_(net[-1].bias)
    return net


def iteration(env, policy, params, steps, lam, L, seed):
    """One forward + backward: returns J [num_envs] (params.grad filled)."""
    env.stop_tape()
    env.reset_sampled("two-stream", seed=seed)
    _, _, per, acts, _, _ = grad.rollout_mlp(env, policy, params, steps)
    J = per.sum(dim=0) + lam * (acts ** 2).sum(dim=(0, 2)) * L / 4
    J.sum().backward()
    return J.detach()


def run(num_envs=64, N=5000, steps=50, iters=10, N_mesh=250, L=50.0, max_mode=5, obs_modes=8, lam=0.1, lr=0.02, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    twin = make(max_mode, obs_modes)
    opt = torch.optim.Adam(twin.parameters(), lr=lr)
    linears = [m for m in twin if isinstance(m, torch.nn.Linear)]
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        policy = MLPPolicy.from_torch(twin, obs_modes)
        params = torch.as_tensor(policy.params, device="cuda").requires_grad_(True)
        J = iteration(env, policy, params, steps, lam, L, seed)
        opt.zero_grad()
        for lin, (gW, gb) in zip(linears, policy.unpack_grad(params.grad)):
            lin.weight.grad = torch.from_numpy(np.ascontiguousarray(gW))
            lin.bias.grad = torch.from_numpy(np.ascontiguousarray(gb))
        opt.step()
        history.append(float(J.mean()))
        print(f"device  iter {it:2d}  J = {history[-1]:.6e}  ({time.perf_counter() - t0:.3f} s)", flush=True)
    env.stop_tape()
    env.close()
    return history


if __name__ == "__main__":
    h = run(*[int(a) for a in sys.argv[1:]])
    print(f"device: J {h[0]:.6e} -> {h[-1]:.6e}")
