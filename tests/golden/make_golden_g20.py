#!/usr/bin/env python3
"""G20: the reference's DeepSets actor (src/control/rl/ddpg.py: Actor -- ParticleEncoder, three Linear -> LayerNorm -> ReLU
layers, a last Linear under a tanh, rescaled to [output_min, output_max] by `sample`) in float64, with the weights and biases of
its five LayerNorms redrawn (uniform +-1.5 / +-1: the defaults 1 / 0 would hide gamma and beta), as G19 does.

Runs ONLY where the reference is available (make_golden.py's `_import_reference`).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_g20.py

Cases (prefix; n_actions = 2M; positions partly outside [0, L), L = 50 the encoder's default period; v_norm = 10 the actor's
default):
  a   mlp_dim = 16, N = 513, M = 3, one environment
  b   mlp_dim = 5,  N = 64,  M = 1, two environments
  c   mlp_dim = 5,  N = 64,  M = 1, two environments, x_norm = 2, output_min / output_max = -0.5 / 2
Stored per case: the state dict's arrays (`<pre>_sd_<name>`), x, v (unnormalised), `mu` = forward(state), `action` =
sample(state), and M, N, mlp_dim, x_norm, v_norm, output_min, output_max.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, save  # noqa: E402

L = 50.0
CASES = (("a", 1, 16, 513, 3, 1.0, -1.0, 1.0), ("b", 2, 5, 64, 1, 1.0, -1.0, 1.0), ("c", 2, 5, 64, 1, 2.0, -0.5, 2.0))
SEED = 2000


def main():
    _import_reference()
    import torch
    from src.control.rl.ddpg import Actor

    out = dict(L=L, cases=np.array([c[0] for c in CASES]))
    for seed, (pre, E, H, N, M, x_norm, lo, hi) in enumerate(CASES):
        torch.manual_seed(SEED + seed)
        rng = np.random.default_rng(SEED + seed)
        actor = Actor(2 * N, H, 2 * M, output_min=lo, output_max=hi, x_norm=x_norm).double()
        v_norm = float(actor.v_norm)
        with torch.no_grad():
            for norm in (actor.encode.phi[1], actor.encode.rho[1], actor.norm1, actor.norm2, actor.norm3):
                norm.weight.uniform_(-1.5, 1.5)
                norm.bias.uniform_(-1.0, 1.0)
        x = torch.tensor(rng.uniform(-0.5 * L, 2.5 * L, (E, N)) * x_norm)
        v = torch.tensor(rng.normal(0.0, 2.0, (E, N)) * v_norm)
        state = torch.cat([x, v], dim=1)
        with torch.no_grad():
            mu, action = actor(state), actor.sample(state)
        out.update({f"{pre}_mlp_dim": H, f"{pre}_N": N, f"{pre}_M": M, f"{pre}_x_norm": x_norm, f"{pre}_v_norm": v_norm,
                    f"{pre}_output_min": lo, f"{pre}_output_max": hi, f"{pre}_x": x.numpy(), f"{pre}_v": v.numpy(),
                    f"{pre}_mu": mu.numpy(), f"{pre}_action": action.numpy()})
        out.update({f"{pre}_sd_{n}": t.numpy() for n, t in actor.state_dict().items()})
    save("g20_particle_actor", **out)


if __name__ == "__main__":
    main()
