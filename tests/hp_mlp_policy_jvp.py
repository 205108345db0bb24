"""Restatement of the device's policy JVP (include/picstep.h: pic_policy_jvp) in NumPy, and the cases the JVP
tests share.  Restatement and test infrastructure only: nothing here is imported by the product.

Every sum is an explicit loop in the header's order, vectorised over environments and output rows: the forward is hp_mlp_policy's;
dy_i = db_i, then for k ascending dy_i = dy_i + dW[i][k] * h[k], then for k ascending dy_i = dy_i + W[i][k] * dh[k], every
product rounded before its sum.  A missing parameter tangent starts dy at +0.0 and leaves the first loop out.
`jvp(..., dtype=np.longdouble)` is the same arithmetic in extended precision; the largest difference between the two over a set
of cases is the floor the tests' tolerance for tanh and squashed networks is derived from (100 x, the rule of DESIGN.md 7c / 7o).
"""
import numpy as np

import hp_mlp_policy as hm
import hp_mlp_policy_vjp as hv
from hp_mlp_policy import M, ENVS, OBS_MODES, make_params, param_count, stacks  # noqa: F401  (the shapes the tests share)


def jvp(widths, activation, params, obs, pre=None, d_params=None, d_obs=None, d_pre=None, squash=False, action_scale=1.0,
        obs_scale=None, dtype=np.float64):
    """(du, da) [E, widths[-1]] of one evaluation per environment and one direction: for observations obs, the recorded pre
    (needed with squash), a parameter tangent d_params ([P], or [E, P] like params; None = 0), an observation tangent d_obs
    [E, widths[0]] (None = 0) and an injection d_pre [E, widths[-1]] in front of the squash (None: none)."""
    f = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    E = np.shape(obs)[0]
    hs = hv.activations(widths, activation, params, obs, obs_scale, dtype)
    layers = hm.layers_of(widths, f(params))
    dlayers = hm.layers_of(widths, f(d_params)) if d_params is not None else None
    dh = f(np.zeros((E, widths[0]))) if d_obs is None else f(d_obs)
    if obs_scale is not None:
        dh = dh * f(obs_scale)
    for l, (W, _) in enumerate(layers):
        h = hs[l]
        nout = W.shape[-2]
        if dlayers is not None:
            dW, db = dlayers[l]
            dy = np.broadcast_to(db, (E, nout)).copy()
            for k in range(W.shape[-1]):
                dy = dy + dW[..., k] * h[:, k:k + 1]
        else:
            dy = f(np.zeros((E, nout)))
        for k in range(W.shape[-1]):
            dy = dy + W[..., k] * dh[:, k:k + 1]
        if l + 1 < len(layers):
            hn = hs[l + 1]
            d = (f(1.0) - hn * hn) if activation == "tanh" else np.where(hn > 0, f(1.0), f(0.0))
            dh = dy * d
    du = dy if d_pre is None else dy + f(d_pre)
    if squash:
        t = np.tanh(f(pre))
        da = (f(action_scale) * (f(1.0) - t * t)) * du
    else:
        da = du
    return du, da


def floor(cases):
    """The largest |float64 - longdouble| of du and da over `cases`, dicts of jvp's keyword arguments."""
    worst = 0.0
    for c in cases:
        u, a = jvp(**c)
        ul, al = jvp(**c, dtype=np.longdouble)
        worst = max(worst, float(np.max(np.abs(u - ul))), float(np.max(np.abs(a - al))))
    return worst


# ---- the cases of tests/test_gpu_policy_jvp.py (pic_policy_jvp against the restatement) --------------------------------------
def jvp_case(E, Mo, widths, activation, squash, seed=0, per_env=False, obs_scale=None):
    """One pic_policy_jvp case and direction: jvp's keyword arguments.  The forward's case (hm.eval_case) plus the three
    tangents; pre is the restatement's own u."""
    c = hm.eval_case(E, Mo, widths, activation, squash, seed=seed, per_env=per_env)
    rng = np.random.default_rng(3000 * seed + 10 * E + Mo + len(widths))
    c = dict(c, obs_scale=obs_scale)
    c["pre"] = hm.forward(**c)[0]
    c["d_params"] = rng.normal(size=np.shape(c["params"]))
    c["d_obs"] = rng.normal(size=(E, widths[0]))
    c["d_pre"] = rng.normal(size=(E, widths[-1]))
    return c


def tanh_cases():
    """The tanh networks and the squashed networks of the JVP test: the cases its tolerance is taken over."""
    out = []
    for E in ENVS:
        for Mo in OBS_MODES:
            for w in stacks(Mo):
                out.append(jvp_case(E, Mo, w, "tanh", False))
                out.append(jvp_case(E, Mo, w, "tanh", True))
                out.append(jvp_case(E, Mo, w, "relu", True))
    return out
