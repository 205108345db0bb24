"""Restatement of the device's policy VJP (include/picstep.h: pic_policy_vjp) in NumPy, and the cases the VJP
tests share.  Restatement and test infrastructure only: nothing here is imported by the product.

Every sum is an explicit loop in the header's order, vectorised over environments and over the index the sum does not run over:
the forward is hp_mlp_policy's (k ascending, the product rounded before the sum); h-bar_l[k] = sum_i W_l[i][k] * delta[i] runs
over i ascending with the first product starting the sum; the parameter terms of one evaluation are single products.
`vjp(..., dtype=np.longdouble)` is the same arithmetic in extended precision; the largest difference between the two over a set
of cases is the floor the tests' tolerance for tanh and squashed networks is derived from (100 x, the rule of DESIGN.md 7c / 7o).
"""
import numpy as np

import hp_mlp_policy as hm
from hp_mlp_policy import M, ENVS, OBS_MODES, make_params, param_count, stacks  # noqa: F401  (the shapes the tests share)


def activations(widths, activation, params, obs, obs_scale=None, dtype=np.float64):
    """h_0 .. h_{L-1} [E, width[l]] as hm.forward computes them (the same operations in the same order)."""
    f = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    h = f(obs)
    if obs_scale is not None:
        h = h * f(obs_scale)
    layers = hm.layers_of(widths, f(params))
    hs = [h]
    for W, b in layers[:-1]:
        y = np.broadcast_to(b, (h.shape[0], b.shape[-1])).copy()
        for k in range(W.shape[-1]):
            y = y + W[..., k] * h[:, k:k + 1]
        h = np.tanh(y) if activation == "tanh" else np.where(y > 0, y, f(0.0))
        hs.append(h)
    return hs


def vjp(widths, activation, params, obs, cot, pre=None, squash=False, action_scale=1.0, obs_scale=None, dtype=np.float64):
    """(g_env [E, P], g_obs [E, widths[0]], g_pre [E, widths[-1]]) of one evaluation per environment: the per-environment
    parameter terms, o-bar and u-bar for observations obs, recorded pre (needed with squash) and the action cotangent cot.
    params [P], or [E, P] with one vector per environment."""
    f = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    E = np.shape(obs)[0]
    hs = activations(widths, activation, params, obs, obs_scale, dtype)
    layers = hm.layers_of(widths, f(params))
    ab = f(cot)
    if squash:
        t = np.tanh(f(pre))
        s = f(action_scale) * (f(1.0) - t * t)
        ub = ab * s
    else:
        ub = ab
    delta = ub
    parts = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        W, _ = layers[l]
        W = np.broadcast_to(W, (E,) + W.shape[-2:])
        h = hs[l]
        gW = delta[:, :, None] * h[:, None, :]
        parts[l] = (gW.reshape(E, -1), delta)
        hb = W[:, 0, :] * delta[:, 0:1]
        for i in range(1, W.shape[1]):
            hb = hb + W[:, i, :] * delta[:, i:i + 1]
        if l > 0:
            d = (f(1.0) - h * h) if activation == "tanh" else np.where(h > 0, f(1.0), f(0.0))
            delta = hb * d
    g_obs = hb * f(obs_scale) if obs_scale is not None else hb
    g_env = np.concatenate([a for pair in parts for a in pair], axis=1)
    return g_env, g_obs, ub


def sum_envs(g_env):
    """[E, P] -> [P]: the environments added in ascending order, the first starting the sum."""
    s = g_env[0].copy()
    for e in range(1, g_env.shape[0]):
        s = s + g_env[e]
    return s


def accumulate(terms):
    """The sum of a list of per-step terms in the list's order (the reverse pass's: t descending), the first starting it."""
    s = terms[0].copy()
    for t in terms[1:]:
        s = s + t
    return s


def floor(cases):
    """The largest |float64 - longdouble| of g_params (per environment and summed), g_obs and g_pre over `cases`, dicts of
    vjp's keyword arguments."""
    worst = 0.0
    for c in cases:
        g, o, u = vjp(**c)
        gl, ol, ul = vjp(**c, dtype=np.longdouble)
        worst = max(worst, float(np.max(np.abs(g - gl))), float(np.max(np.abs(o - ol))), float(np.max(np.abs(u - ul))),
                    float(np.max(np.abs(sum_envs(g) - sum_envs(gl)))))
    return worst


# ---- the cases of tests/test_gpu_policy_vjp.py (pic_policy_vjp against the restatement) --------------------------------------
def vjp_case(E, Mo, widths, activation, squash, seed=0, per_env=False, obs_scale=None):
    """One pic_policy_vjp case: vjp's keyword arguments.  The forward's case (hm.eval_case) plus a cotangent; pre is the
    restatement's own u."""
    c = hm.eval_case(E, Mo, widths, activation, squash, seed=seed, per_env=per_env)
    rng = np.random.default_rng(2000 * seed + 10 * E + Mo + len(widths))
    c = dict(c, cot=rng.normal(size=(E, widths[-1])), obs_scale=obs_scale)
    c["pre"] = hm.forward(**{k: v for k, v in c.items() if k != "cot"})[0]
    return c


def tanh_cases():
    """The tanh networks and the squashed networks of the VJP test: the cases its tolerance is taken over."""
    out = []
    for E in ENVS:
        for Mo in OBS_MODES:
            for w in stacks(Mo):
                out.append(vjp_case(E, Mo, w, "tanh", False))
                out.append(vjp_case(E, Mo, w, "tanh", True))
                out.append(vjp_case(E, Mo, w, "relu", True))
    return out
