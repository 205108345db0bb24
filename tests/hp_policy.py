"""Oracle of a closed loop under a generic policy: a_t = pi(o_t), restated in float64 torch on the CPU on top of
the Yoshida-4 step of tests/hp_adjoint.py and differentiated by autograd.

The observation o_t is either the modes of the field step t starts from, m_t = J E_t with J of M_o rows (tests/hp_feedback.py:
jacobian; o_0 reads the field of x_0), or the state (x_t, v_t) itself.  The actions drive the actuator field B a_t
(hp_feedback.basis).  The policies below take parameters with the same leading axes as their observation, so that one set of
parameters per environment gives a device gradient per environment: p[e] is environment e's alone.
"""
import numpy as np
import torch

import hp_adjoint as ha
import hp_feedback as hf


def rollout(x0, v0, policy, S, T, M, observe="modes", obs_modes=None):
    """T closed-loop steps of one environment from (x0, v0) under a_t = policy(o_t).  Returns hist [T, 3] (KE, PE, PE_reward),
    actions [T, 2M] and the observations o_0..o_T."""
    Mo = M if obs_modes is None else int(obs_modes)
    J = torch.as_tensor(hf.jacobian(S.Ng, Mo))
    B = torch.as_tensor(hf.basis(S.L, S.Ng, M))
    x, v = x0, v0
    E = ha.field(ha.density(x0, S), S)
    obs = [J @ E if observe == "modes" else (x, v)]
    hist, acts = [], []
    for _ in range(T):
        a = policy(obs[-1]).to(torch.float64)
        x, v, ke, pe, per, E = ha.step(x, v, B @ a, S)
        hist.append(torch.stack([ke, pe, per]))
        acts.append(a)
        obs.append(J @ E if observe == "modes" else (x, v))
    return torch.stack(hist), torch.stack(acts), obs


# ---- policies whose parameters may carry leading environment axes -----------------------------------------------------------
def mlp_params(n_in, n_out, hidden, lead=(), seed=0, scale=0.5):
    """Parameters of mlp_modes: W1 [*lead, H, n_in], b1 [*lead, H], W2 [*lead, n_out, H], b2 [*lead, n_out] (float64)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*lead, *s, generator=g, dtype=torch.float64)
    return {"W1": r(hidden, n_in) * scale, "b1": r(hidden) * 0.1, "W2": r(n_out, hidden) * scale, "b2": r(n_out) * 0.1}


def mlp_modes(p, m):
    """A two-layer tanh MLP on the modes m [..., 2 M_o] -> actions [..., 2M]."""
    h = torch.tanh(torch.einsum("...hi,...i->...h", p["W1"], m) + p["b1"])
    return torch.einsum("...oh,...h->...o", p["W2"], h) + p["b2"]


def deepsets_params(n_out, hidden, lead=(), seed=0, scale=0.5):
    """Parameters of deepsets_state: phi (W1 [*lead, H, 3], b1) and rho (W2 [*lead, n_out, H], b2)."""
    return mlp_params(3, n_out, hidden, lead, seed, scale)


def deepsets_state(p, xv, L):
    """The reference's DeepSets encoder shape: per particle phi(cos q, sin q, p) with q = 2 pi x / L, mean over particles,
    then rho -> actions [..., 2M].  xv = (x, v), each [..., N]."""
    x, v = xv
    q = 2 * np.pi * x / L
    f = torch.stack([torch.cos(q), torch.sin(q), v], dim=-1)                       # [..., N, 3]
    h = torch.tanh(torch.einsum("...nk,...hk->...nh", f, p["W1"]) + p["b1"].unsqueeze(-2))
    return torch.einsum("...oh,...h->...o", p["W2"], h.mean(dim=-2)) + p["b2"]


def loss_terms(hist, acts, obs, w_hist, w_act=0.0, w_obs=None):
    """<w_hist, hist> + w_act sum a^2 (+ <w_obs, o_T> for modes): a cost built from the traces, as the examples build theirs."""
    J = (hist * torch.as_tensor(np.asarray(w_hist, dtype=np.float64))).sum() + w_act * (acts ** 2).sum()
    if w_obs is not None:
        J = J + (obs[-1] * torch.as_tensor(np.asarray(w_obs, dtype=np.float64))).sum()
    return J
