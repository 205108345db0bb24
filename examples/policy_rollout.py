"""On-policy data collection on the device: a Gaussian MLP policy on the Fourier modes of the field, whole rollouts in one
call each (BatchedPIC.step_policy -> pic_step_policy), and a policy-gradient update of its torch twin.

Every iteration
  1. draws one noise tensor for the whole rollout (torch.randn: the library has no RNG) and collects T steps of every
     environment with step_policy: observations, pre-squash actions u = mean + std * eps, actions and energies come back at once;
  2. computes the trainers' reward (Reward.compute_reward, the formula of BatchedPIC.trainer_rewards_torch) of every step from
     the PE_reward of the state the step started from and the action it ran under;
  3. updates the torch twin (MLPPolicy.to_torch) by the score-function gradient of the discounted returns-to-go, with their
     mean over the environments as the baseline of each time step;
  4. repacks the twin's weights for the next collection (MLPPolicy.from_torch).

Prints the mean return per iteration (of at most 2 per step; with the defaults 50.4 -> 53.7 over 40 iterations, 2.2 ms per
collection of 50 x 256 steps on an MI355X).

    python examples/policy_rollout.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.control.policy import MLPPolicy  # noqa: E402


def rewards(per_before, actions, L, alpha=1.0, beta=1.0, r_pe_n=1.0):
    """trainer_rewards_torch's formula for a whole rollout: per_before [T, E] the field energy of the state each step started
    from, actions [T, E, A] what it ran under."""
    ie = (actions * actions).sum(dim=2) * (L * 0.25)
    r_ie_n = actions.shape[2] * L * 0.25
    return alpha * torch.clamp(1.0 - per_before / r_pe_n, min=0.0) + beta * torch.clamp(1.0 - ie / r_ie_n, min=0.0)


def run(num_envs=256, N=5000, steps=50, iters=40, N_mesh=250, L=50.0, max_mode=3, obs_modes=3, hidden=64, sigma=0.1,
        action_scale=1.25, gamma=0.98, lr=1e-2, seed=3):
    dev = "cuda"
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    torch.manual_seed(0)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(2 * obs_modes, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                        nn.Linear(hidden, 2 * max_mode), nn.Tanh()).double()
    obs_scale = torch.full((2 * obs_modes,), 8.0, dtype=torch.float64)
    policy = MLPPolicy.from_torch(net, obs_modes, action_scale=action_scale, obs_scale=obs_scale)
    twin = policy.to_torch().to(dev)                    # the module the optimiser owns
    opt = torch.optim.Adam(twin.parameters(), lr=lr)
    std = torch.full((2 * max_mode,), sigma, dtype=torch.float64, device=dev)
    disc = gamma ** torch.arange(steps, dtype=torch.float64, device=dev)
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        env.reset_sampled("two-stream", seed=seed)          # the same ensemble every iteration: only the noise differs
        per0 = torch.as_tensor(env.energies()[2], device=dev)
        eps = torch.randn((steps, num_envs, 2 * max_mode), dtype=torch.float64, device=dev)
        roll = env.step_policy(policy, steps, noise=eps, std=std, history=True, on_device=True)
        t_collect = time.perf_counter() - t0
        per = torch.as_tensor(roll.PE_reward, device=dev)
        r = rewards(torch.cat([per0[None], per[:-1]]), roll.actions, L)
        # discounted returns-to-go against a baseline per time step (their mean over the environments), normalised
        G = torch.flip(torch.cumsum(torch.flip(r * disc[:, None], [0]), 0), [0]) / disc[:, None]
        adv = G - G.mean(dim=1, keepdim=True)
        adv = adv / (adv.std() + 1e-12)
        # score function of u ~ N(mean(o), std): the twin without its final Tanh gives the mean of the pre-squash action
        mean = twin[:-1](roll.obs * obs_scale.to(dev))
        logp = (-0.5 * ((roll.pre - mean) / std) ** 2).sum(dim=2)
        loss = -(adv * logp).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        policy = MLPPolicy.from_torch(twin, obs_modes, action_scale=action_scale, obs_scale=obs_scale)      # repack
        history.append(float(r.sum(dim=0).mean()))
        print(f"iter {it:2d}  return = {history[-1]:.4f}  collect {1e3 * t_collect:.1f} ms for {steps} x {num_envs} steps  "
              f"iteration {time.perf_counter() - t0:.3f} s", flush=True)
    env.close()
    return history


if __name__ == "__main__":
    h = run(*[int(a) for a in sys.argv[1:]])
    print(f"return {h[0]:.4f} -> {h[-1]:.4f}")
