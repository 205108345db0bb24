#!/usr/bin/env python3
"""G19: the reference's DeepSets particle encoder (src/control/rl/encode.py: ParticleEncoder, phi = Linear(3, H) -> LayerNorm(H)
-> ReLU, the mean over the particles, rho = Linear(H, H_out) -> LayerNorm(H_out) -> ReLU) in float64, with the weights and
biases of its two LayerNorms redrawn (uniform +-1.5 / +-1: the defaults 1 / 0 would hide gamma and beta).

Runs ONLY where the reference is available (make_golden.py's `_import_reference`).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_g19.py

Cases (prefix; two environments each but for a, which has one; positions partly outside [0, L), L = 50 the encoder's default period):
  a   H = 16, H_out = 8, N = 513
  b   H = 5,  H_out = 3, N = 64
  c   H = 1,  H_out = 2, N = 5
  d   H = 5,  H_out = 3, N = 64 with x_norm = 2, v_norm = 10 applied the way Actor.forward (ddpg.py:106-109) applies them: the
      encoder is fed cat(x / x_norm, v / v_norm)
Stored per case: the state dict's arrays (`<pre>_sd_<name>`), x, v (unnormalised), `phi_mean` = phi(z).mean(1), `enc` = the
encoder's output, a cotangent `cot_phi` on phi_mean with torch autograd's gradients of <cot_phi, phi_mean> with respect to x, v
and phi's four tensors (`gphi_*`), and a cotangent `cot_enc` on the output with the gradients of <cot_enc, enc> with respect to
x, v and all eight tensors (`genc_*`).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, save  # noqa: E402

L = 50.0
CASES = (("a", 1, 16, 8, 513, 1.0, 1.0), ("b", 2, 5, 3, 64, 1.0, 1.0), ("c", 2, 1, 2, 5, 1.0, 1.0), ("d", 2, 5, 3, 64, 2.0, 10.0))


def main():
    _import_reference()
    import torch
    from src.control.rl.encode import ParticleEncoder

    out = dict(L=L, cases=np.array([c[0] for c in CASES]))
    for seed, (pre, E, H, H_out, N, x_norm, v_norm) in enumerate(CASES):
        torch.manual_seed(1900 + seed)
        rng = np.random.default_rng(1900 + seed)
        enc = ParticleEncoder(H, H_out).double()
        with torch.no_grad():
            for norm in (enc.phi[1], enc.rho[1]):
                norm.weight.uniform_(-1.5, 1.5)
                norm.bias.uniform_(-1.0, 1.0)
        x = torch.tensor(rng.uniform(-0.5 * L, 2.5 * L, (E, N)) * x_norm, requires_grad=True)
        v = torch.tensor(rng.normal(0.0, 2.0, (E, N)) * v_norm, requires_grad=True)
        state = torch.cat([x / x_norm, v / v_norm], dim=1)
        # phi(z).mean(1) the way ParticleEncoder.forward forms it
        q, p = state[:, :N], state[:, N:]
        z = torch.stack([torch.cos(q * 2 * torch.pi / enc.L), torch.sin(q * 2 * torch.pi / enc.L), p], dim=-1)
        phi_mean = enc.phi(z).mean(dim=1)
        y = enc(state)
        assert torch.equal(enc.rho(phi_mean), y)
        cot_phi, cot_enc = torch.tensor(rng.normal(0.0, 1.0, (E, H))), torch.tensor(rng.normal(0.0, 1.0, (E, H_out)))
        names = list(enc.state_dict())
        params = dict(enc.named_parameters())
        phi_names = [n for n in names if n.startswith("phi.")]
        gphi = torch.autograd.grad((phi_mean * cot_phi).sum(), [x, v] + [params[n] for n in phi_names], retain_graph=True)
        genc = torch.autograd.grad((y * cot_enc).sum(), [x, v] + [params[n] for n in names])
        out.update({f"{pre}_H": H, f"{pre}_H_out": H_out, f"{pre}_N": N, f"{pre}_x_norm": x_norm, f"{pre}_v_norm": v_norm,
                    f"{pre}_x": x.detach().numpy(), f"{pre}_v": v.detach().numpy(), f"{pre}_phi_mean": phi_mean.detach().numpy(),
                    f"{pre}_enc": y.detach().numpy(), f"{pre}_cot_phi": cot_phi.numpy(), f"{pre}_cot_enc": cot_enc.numpy()})
        out.update({f"{pre}_sd_{n}": t.numpy() for n, t in enc.state_dict().items()})
        out.update({f"{pre}_gphi_{n}": g.numpy() for n, g in zip(["x", "v"] + phi_names, gphi)})
        out.update({f"{pre}_genc_{n}": g.numpy() for n, g in zip(["x", "v"] + names, genc)})
    save("g19_particle_encoder", **out)


if __name__ == "__main__":
    main()
