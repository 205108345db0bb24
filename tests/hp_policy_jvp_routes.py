"""The two older routes the device's forward mode through an MLP policy is measured against, for one MLPPolicy with
noise: env.grad.rollout_policy_jvp under the policy's float64 torch twin on the device (back in Python every step), and torch
forward mode of tests/hp_policy.py's rollout on the CPU.  Test infrastructure only: nothing here is imported by the product.

The twin is written out as a function fn(params, o) of a dict of tensors (W0, b0, ..., std), so that a direction in the packed
parameters and in std is a dict of the same names.  The noise of step t is picked by counting fn's calls: rollout_policy_jvp calls
it once per step of the forward (T calls), then once per step and direction in the walk; hp_policy.rollout once per step.
"""
import numpy as np
import torch

import hp_adjoint as ha
import hp_tangent_walk as hw


class Twin:
    def __init__(self, pol, eps, std):
        self.pol, self.eps, self.std = pol, np.asarray(eps), np.asarray(std)
        self.L = len(pol.widths) - 1

    def _dict(self, flat, std, device):
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)  # noqa: E731
        d = {}
        for l, (W, b) in enumerate(self.pol.unpack(np.asarray(flat))):
            d[f"W{l}"], d[f"b{l}"] = t(W), t(b)
        d["std"] = t(std)
        return d

    def params(self, device):
        return self._dict(np.asarray(self.pol.params), self.std, device)

    def direction(self, d_params, d_std, device):
        return self._dict(d_params, d_std, device)

    def fn(self, T, K, device, env=None):
        """fn(params, o): o [E, 2 M_o] (env None) or the observation [2 M_o] of environment `env` alone."""
        pol, calls = self.pol, [0]
        eps = torch.as_tensor(self.eps if env is None else self.eps[:, env], dtype=torch.float64, device=device)
        scale = None if pol.obs_scale is None else torch.as_tensor(np.asarray(pol.obs_scale), dtype=torch.float64, device=device)

        def fn(p, o):
            c = calls[0]
            calls[0] += 1
            t = c if c < T else (c - T) // K
            h = o if scale is None else o * scale
            for l in range(self.L):
                y = h @ p[f"W{l}"].T + p[f"b{l}"]
                h = y if l + 1 == self.L else (torch.tanh(y) if pol.activation == "tanh" else torch.relu(y))
            u = h + p["std"] * eps[t]
            return pol.action_scale * torch.tanh(u) if pol.squash else u

        return fn


def twin_route(env, twin, d_params, d_std, T, d_x0=None, d_v0=None, checkpoint_every=0):
    """rollout_policy_jvp on `env` (freshly reset) under the twin: K directions (d_params [K, P], d_std [K, 2M], d_x0 / d_v0
    [K, E, N] or None) -> its dict, as NumPy arrays."""
    from ocplasma_amd.env import grad
    K = len(d_params)
    dps = [twin.direction(d_params[k], d_std[k], "cuda") for k in range(K)]
    out = grad.rollout_policy_jvp(env, twin.fn(T, K, "cuda"), twin.params("cuda"), dps, T, observe="modes",
                                  obs_modes=twin.pol.obs_modes, d_x0=d_x0, d_v0=d_v0, checkpoint_every=checkpoint_every)
    return {k: v.detach().cpu().numpy() for k, v in out.items() if k != "obs"}


def oracle_route(X, V, twin, d_params, d_std, T, Ng, L, dt, M, d_x0=None, d_v0=None):
    """torch forward mode of hp_policy.rollout on the CPU, environment by environment and direction by direction ->
    d_hist [K, T, 3, E], d_actions [K, T, E, 2M]."""
    E, N = X.shape
    K = len(d_params)
    S = ha.Setup(N, Ng, L, 1.0, dt)
    hist, acts = np.zeros((K, T, 3, E)), np.zeros((K, T, E, 2 * M))
    for k in range(K):
        dp = {n: a.numpy() for n, a in twin.direction(d_params[k], d_std[k], "cpu").items()}
        for e in range(E):
            h, a = hw.torch_policy_jvp(X[e], V[e], twin.fn(T, 1, "cpu", env=e), twin.params("cpu"), dp, S, T, M, "modes",
                                       twin.pol.obs_modes, d_x0=None if d_x0 is None else d_x0[k, e],
                                       d_v0=None if d_v0 is None else d_v0[k, e])
            hist[k, :, :, e], acts[k, :, e] = h, a
    return hist, acts
