"""Restatement of the device's MLP policy (include/picstep.h: pic_policy) in NumPy, and the cases the policy tests
share.  Restatement and test infrastructure only: nothing here is imported by the product.

A layer is y_i = b_i, then for k ascending y_i = y_i + W[i][k] * h[k] with the product rounded before the sum: an explicit loop
over k (np.dot sums in another order), vectorised over environments and outputs.  `forward(..., dtype=np.longdouble)` is the same
arithmetic in extended precision; the largest difference between the two over a set of cases is the floor the tests' tolerance
for tanh networks is derived from (100 x, the rule of DESIGN.md 7c): the device's tanh and NumPy's may differ in the last bits.
"""
import numpy as np


def param_count(widths):
    return sum(widths[l + 1] * widths[l] + widths[l + 1] for l in range(len(widths) - 1))


def make_params(widths, seed, lead=()):
    """A parameter vector [*lead, P]: W ~ N(0, 1 / in), b ~ 0.1 N(0, 1)."""
    rng = np.random.default_rng(seed)
    parts = []
    for l in range(len(widths) - 1):
        nin, nout = widths[l], widths[l + 1]
        parts.append(rng.normal(size=lead + (nout * nin,)) / np.sqrt(nin))
        parts.append(0.1 * rng.normal(size=lead + (nout,)))
    return np.concatenate(parts, axis=-1)


def layers_of(widths, params):
    """[(W [*lead, out, in], b [*lead, out])] views of a parameter vector [*lead, P]."""
    p = np.asarray(params)
    lead, out, at = p.shape[:-1], [], 0
    for l in range(len(widths) - 1):
        nin, nout = widths[l], widths[l + 1]
        W = p[..., at:at + nout * nin].reshape(*lead, nout, nin)
        at += nout * nin
        out.append((W, p[..., at:at + nout]))
        at += nout
    assert at == p.shape[-1]
    return out


def forward(widths, activation, params, obs, noise=None, std=None, squash=False, action_scale=1.0, obs_scale=None,
            dtype=np.float64):
    """(pre, actions) [E, widths[-1]] of observations obs [E, widths[0]]; params [P], or [E, P] with one vector per environment.
    Every operation is a single rounded NumPy operation of `dtype`, in the device's order."""
    f = lambda a: np.asarray(a, dtype=dtype)
    h = f(obs)
    if obs_scale is not None:
        h = h * f(obs_scale)
    layers = layers_of(widths, f(params))
    for l, (W, b) in enumerate(layers):
        y = np.broadcast_to(b, (h.shape[0], b.shape[-1])).copy()
        for k in range(W.shape[-1]):
            y = y + W[..., k] * h[:, k:k + 1]
        if l + 1 < len(layers):
            y = np.tanh(y) if activation == "tanh" else np.where(y > 0, y, f(0.0))
        h = y
    u = h
    if noise is not None:
        sd = f(np.ones(widths[-1])) if std is None else f(std)
        u = h + sd * f(noise)
    a = f(action_scale) * np.tanh(u) if squash else u
    return u, a


def floor(cases):
    """The largest |float64 - longdouble| of pre and actions over `cases`, dicts of forward's keyword arguments."""
    worst = 0.0
    for c in cases:
        u, a = forward(**c)
        ul, al = forward(**c, dtype=np.longdouble)
        worst = max(worst, float(np.max(np.abs(u - ul))), float(np.max(np.abs(a - al))))
    return worst


# ---- the shapes of tests/test_gpu_policy.py (policy_eval against the restatement) -------------------------------------------
M = 2                                  # actuator modes: 2M = 4 actions
ENVS = (1, 3)
OBS_MODES = (2, 5)


def stacks(Mo):
    return ([2 * Mo, 2 * M], [2 * Mo, 37, 5, 2 * M], [2 * Mo, 256, 256, 256, 2 * M])


def eval_case(E, Mo, widths, activation, squash, seed=0, per_env=False):
    """One policy_eval case on a given observation: forward's keyword arguments."""
    rng = np.random.default_rng(1000 * seed + 10 * E + Mo + len(widths))
    return dict(widths=widths, activation=activation, params=make_params(widths, seed + 1, (E,) if per_env else ()),
                obs=0.5 * rng.normal(size=(E, 2 * Mo)), squash=squash, action_scale=1.25 if squash else 1.0)


def tanh_cases():
    """The tanh networks and the squashed relu networks of the policy_eval test: the cases its tolerance is taken over."""
    out = []
    for E in ENVS:
        for Mo in OBS_MODES:
            for w in stacks(Mo):
                out.append(eval_case(E, Mo, w, "tanh", False))
                out.append(eval_case(E, Mo, w, "tanh", True))
                out.append(eval_case(E, Mo, w, "relu", True))
    return out
