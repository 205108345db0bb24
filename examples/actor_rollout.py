"""Data collection under the DeepSets particle actor on the device (BatchedPIC.step_actor -> pic_step_actor), one
gradient step on its torch twin through the existing differentiable route, and collection again under the updated actor.

  1. load an actor from a state dict (ParticleActor.from_reference: `encode.phi.*`, `encode.rho.*`, `fc1`/`norm1` .. `fc3`/
     `norm3`, `fc_out`; a torch.save'd file given with --state-dict) or draw one of that shape;
  2. collect T closed-loop steps of every environment in ONE call: pooled features, pre-squash actions, actions and energies of
     every step come back at once (the noise is the caller's: the library has no RNG);
  3. take one gradient step on the twin (ParticleActor.to_torch: PoolEncoder + torch layers on (x, v)) with
     env.grad.rollout_policy(observe="state") over a short horizon: the cost is the field energy the steps leave;
  4. repack the twin (ParticleActor.with_torch) and collect again.

    python examples/actor_rollout.py [--envs 64] [--N 5000] [--steps 50] [--grad-steps 5] [--hidden 64] [--state-dict FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.control.actor import ParticleActor  # noqa: E402
from ocplasma_amd.env import grad  # noqa: E402


def drawn_state_dict(H, n_actions, seed=0):
    """A state dict of the reference actor's shape (mlp_dim H) with PyTorch's default initialisation."""
    torch.manual_seed(seed)
    nn = torch.nn
    mods = {"encode.phi.0": nn.Linear(3, H), "encode.phi.1": nn.LayerNorm(H), "encode.rho.0": nn.Linear(H, H),
            "encode.rho.1": nn.LayerNorm(H), "fc_out": nn.Linear(H, n_actions)}
    for i in (1, 2, 3):
        mods[f"fc{i}"], mods[f"norm{i}"] = nn.Linear(H, H), nn.LayerNorm(H)
    return {f"{k}.{n}": p.detach().double().numpy() for k, m in mods.items() for n, p in m.named_parameters()}


def run(num_envs=64, N=5000, steps=50, grad_steps=5, hidden=64, state_dict=None, N_mesh=250, L=50.0, max_mode=3, sigma=0.1, lr=1e-2,
        seed=3):
    dev = "cuda"
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    sd = torch.load(state_dict, map_location="cpu") if state_dict else drawn_state_dict(hidden, 2 * max_mode)
    actor = ParticleActor.from_reference(sd, L_ref=L, x_norm=1.0, v_norm=10.0, output_min=-1.0, output_max=1.0)
    std = torch.full((2 * max_mode,), sigma, dtype=torch.float64, device=dev)

    def collect(actor):
        env.reset_sampled("two-stream", seed=seed)
        eps = torch.randn((steps, num_envs, 2 * max_mode), dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        roll = env.step_actor(actor, steps, noise=eps, std=std, history=True, on_device=True)
        ms = 1e3 * (time.perf_counter() - t0)
        print(f"collected {steps} x {num_envs} steps in {ms:.1f} ms: features {tuple(roll.features.shape)}, actions "
              f"{tuple(roll.actions.shape)}, mean field energy {float(np.mean(roll.PE_reward)):.6f}, bad {env.bad_count()}", flush=True)
        return roll

    first = collect(actor)
    # one gradient step on the twin, through the pooled features' VJP and the tape's reverse walk
    twin = actor.to_torch(env)
    opt = torch.optim.Adam(twin.parameters(), lr=lr)
    env.reset_sampled("two-stream", seed=seed)
    ke, pe, per, acts, _ = grad.rollout_policy(env, twin, grad_steps, observe="state")
    loss = per.mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    env.stop_tape()                                     # (rollout_policy's tape: step_actor is refused while one is open)
    print(f"twin: field energy over {grad_steps} steps {float(loss.detach()):.6f}; |grad| = "
          f"{float(torch.sqrt(sum((p.grad ** 2).sum() for p in twin.parameters()))):.3e}", flush=True)
    second = collect(actor.with_torch(twin))
    env.close()
    return first, second


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--N", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--grad-steps", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--state-dict", default=None)
    a = ap.parse_args()
    run(a.envs, a.N, a.steps, a.grad_steps, a.hidden, a.state_dict)
