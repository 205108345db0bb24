"""Restatement of the particle actor's head (include/picstep.h: pic_actor) in NumPy, and the cases the actor tests
share.  Restatement and test infrastructure only: nothing here is imported by the product.

A layer is y_i = b_i, then for k ascending y_i = y_i + W[i][k] * h[k] with the product rounded before the sum; the LayerNorm's two
sums run from +0 over ascending i: explicit loops (np.dot and np.mean sum in another order), vectorised over the environments.
`forward(..., dtype=np.longdouble)` is the same arithmetic in extended precision; the largest difference between the two over a
set of cases is the floor the tolerances are derived from (100 x, the rule of DESIGN.md 7c): the device's tanh and NumPy's may
differ in the last bits.  The pooled features in front of the head are tests/hp_pool.py's and tests/hp_pool_ln.py's.
"""
import functools
import os

import numpy as np

import hp_pool_ln as hl

LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_particle_actor.npz")


def param_count(widths, layernorm):
    n = len(widths) - 1
    return sum(widths[l + 1] * widths[l] + widths[l + 1] + (2 * widths[l + 1] if layernorm and l + 1 < n else 0) for l in range(n))


def make_params(widths, layernorm, seed, lead=()):
    """A parameter vector [*lead, P]: W ~ N(0, 1 / in), b ~ 0.1 N(0, 1), gamma ~ U(-1.5, 1.5), beta ~ U(-1, 1)."""
    rng = np.random.default_rng(seed)
    parts, n = [], len(widths) - 1
    for l in range(n):
        nin, nout = widths[l], widths[l + 1]
        parts.append(rng.normal(size=lead + (nout * nin,)) / np.sqrt(nin))
        parts.append(0.1 * rng.normal(size=lead + (nout,)))
        if layernorm and l + 1 < n:
            parts.append(rng.uniform(-1.5, 1.5, size=lead + (nout,)))
            parts.append(rng.uniform(-1.0, 1.0, size=lead + (nout,)))
    return np.concatenate(parts, axis=-1)


def layers_of(widths, layernorm, params):
    """[(W [*lead, out, in], b, gamma, beta [*lead, out])] views of a parameter vector [*lead, P] (gamma, beta None without)."""
    p = np.asarray(params)
    lead, out, at, n = p.shape[:-1], [], 0, len(widths) - 1
    for l in range(n):
        nin, nout = widths[l], widths[l + 1]
        W = p[..., at:at + nout * nin].reshape(*lead, nout, nin)
        at += nout * nin
        b = p[..., at:at + nout]
        at += nout
        g = be = None
        if layernorm and l + 1 < n:
            g, be = p[..., at:at + nout], p[..., at + nout:at + 2 * nout]
            at += 2 * nout
        out.append((W, b, g, be))
    assert at == p.shape[-1]
    return out


def forward(widths, layernorm, activation, params, features, noise=None, std=None, squash=False, action_scale=1.0,
            action_shift=0.0, ln_eps=1e-5, dtype=np.float64):
    """(pre, actions) [E, widths[-1]] of features [E, widths[0]]; params [P], or [E, P] with one vector per environment.  Every
    operation is a single rounded NumPy operation of `dtype`, in the device's order."""
    f = lambda a: np.asarray(a, dtype=dtype)
    h = f(features)
    E = h.shape[0]
    layers = layers_of(widths, layernorm, f(params))
    for l, (W, b, g, be) in enumerate(layers):
        n = b.shape[-1]
        y = np.broadcast_to(b, (E, n)).copy()
        for k in range(W.shape[-1]):
            y = y + W[..., k] * h[:, k:k + 1]
        if l + 1 < len(layers):
            if layernorm:
                s = np.zeros(E, dtype=dtype)
                for i in range(n):
                    s = s + y[:, i]
                mu = s / f(n)
                d = y - mu[:, None]
                q = np.zeros(E, dtype=dtype)
                for i in range(n):
                    q = q + d[:, i] * d[:, i]
                r = f(1.0) / np.sqrt(q / f(n) + f(ln_eps))
                y = g * (d * r[:, None]) + be
            y = np.tanh(y) if activation == "tanh" else np.where(y > 0, y, f(0.0))
        h = y
    u = h
    if noise is not None:
        sd = f(np.ones(widths[-1])) if std is None else f(std)
        u = h + sd * f(noise)
    a = f(action_shift) + f(action_scale) * np.tanh(u) if squash else u
    return u, a


def action_unit(c):
    return max(1.0, abs(c.get("action_scale", 1.0)) + abs(c.get("action_shift", 0.0))) if c.get("squash") else 1.0


def floor(cases):
    """The largest |float64 - longdouble| of pre, and of actions relative to max(1, |action_scale| + |action_shift|), over
    `cases`, dicts of forward's keyword arguments."""
    worst = 0.0
    for c in cases:
        u, a = forward(**c)
        ul, al = forward(**c, dtype=LD)
        worst = max(worst, float(np.max(np.abs(u - ul))), float(np.max(np.abs(a - al))) / action_unit(c))
    return worst


# ---- the shapes of tests/test_gpu_actor.py (actor_eval on given features against the restatement) -----------------------------
def stacks(H, M):
    return ([H, 2 * M], [H, 37, 1, 2 * M], [H, 256, 256, 256, 256, 256, 2 * M])


# a sample of the product E x H x head x layernorm x activation x per_env x M (every value of every factor appears)
EVAL_CASES = (
    # E, H, head, layernorm, activation, per_env, M, squash
    (1, 1, 0, False, "tanh", False, 1, False),
    (3, 1, 1, True, "relu", True, 3, True),
    (1, 5, 1, True, "tanh", False, 3, True),
    (3, 5, 2, False, "relu", False, 1, True),
    (3, 64, 0, True, "relu", True, 1, False),
    (1, 64, 2, True, "relu", False, 3, True),
    (3, 64, 1, False, "tanh", True, 3, False),
    (1, 256, 2, True, "tanh", True, 1, True),
    (3, 256, 0, False, "relu", False, 3, True),
    (3, 256, 1, True, "relu", False, 1, False),
)


def eval_case(E, H, head, layernorm, activation, per_env, M, squash, seed=0):
    """One actor_eval case on given features: forward's keyword arguments."""
    widths = stacks(H, M)[head]
    rng = np.random.default_rng(1000 * seed + 10 * E + H + len(widths))
    return dict(widths=widths, layernorm=layernorm, activation=activation,
                params=make_params(widths, layernorm, seed + 1, (E,) if per_env else ()), features=rng.uniform(0.0, 1.0, (E, H)),
                noise=rng.normal(size=(E, 2 * M)), std=rng.uniform(0.05, 0.3, 2 * M), squash=squash,
                action_scale=1.25 if squash else 1.0, action_shift=0.75 if squash else 0.0, ln_eps=1e-5)


@functools.lru_cache(maxsize=None)
def eval_floor():
    return floor([eval_case(*c) for c in EVAL_CASES])


# ---- g20: the reference's actor (tests/golden/make_golden_g20.py) -----------------------------------------------------------------
G20_CASES = ("a", "b", "c")


@functools.lru_cache(maxsize=None)
def g20():
    return dict(np.load(GOLDEN))


def g20_state_dict(pre):
    tag = f"{pre}_sd_"
    return {k[len(tag):]: a for k, a in g20().items() if k.startswith(tag)}


def g20_head(pre):
    """(widths, params, kwargs) of the case's head in the device's layout, and its pool part."""
    sd, g = g20_state_dict(pre), g20()
    layers = [(sd["encode.rho.0.weight"], sd["encode.rho.0.bias"], sd["encode.rho.1.weight"], sd["encode.rho.1.bias"])]
    layers += [(sd[f"fc{i}.weight"], sd[f"fc{i}.bias"], sd[f"norm{i}.weight"], sd[f"norm{i}.bias"]) for i in (1, 2, 3)]
    parts = []
    for W, b, ga, be in layers:
        parts += [W.ravel(), b, ga, be]
    parts += [sd["fc_out.weight"].ravel(), sd["fc_out.bias"]]
    widths = [layers[0][0].shape[1]] + [t[0].shape[0] for t in layers] + [sd["fc_out.weight"].shape[0]]
    lo, hi = float(g[f"{pre}_output_min"]), float(g[f"{pre}_output_max"])
    kw = dict(widths=widths, layernorm=True, activation="relu", params=np.concatenate(parts), squash=True,
              action_scale=(hi - lo) / 2, action_shift=(hi + lo) / 2, ln_eps=1e-5)
    pool = dict(W=sd["encode.phi.0.weight"], b=sd["encode.phi.0.bias"], gamma=sd["encode.phi.1.weight"], beta=sd["encode.phi.1.bias"],
                period=float(g["L"]) * float(g[f"{pre}_x_norm"]), v_scale=1.0 / float(g[f"{pre}_v_norm"]))
    return kw, pool


def g20_restated(pre, dtype=np.float64):
    """(pre, actions) of the case: the pooled features' restatement (hp_pool_ln), then the head's; dtype LD: both twins."""
    g = g20()
    kw, p = g20_head(pre)
    X, V = g[f"{pre}_x"], g[f"{pre}_v"]
    if dtype is LD:
        feats = np.stack([hl.both_ld(x, v, p["W"], p["b"], p["gamma"], p["beta"], None, p["period"], "relu", p["v_scale"])[0]
                          for x, v in zip(X, V)])
    else:
        feats = np.stack([hl.forward(x, v, p["W"], p["b"], p["gamma"], p["beta"], p["period"], "relu", p["v_scale"]) for x, v in zip(X, V)])
    return forward(features=feats, dtype=dtype, **kw), kw


@functools.lru_cache(maxsize=None)
def g20_floor():
    """The largest float64 - longdouble difference of the whole restated chain over the g20 cases (pre, and actions relative to
    max(1, |action_scale| + |action_shift|))."""
    worst = 0.0
    for pre in G20_CASES:
        (u, a), kw = g20_restated(pre)
        (ul, al), _ = g20_restated(pre, LD)
        worst = max(worst, float(np.max(np.abs(u - ul))), float(np.max(np.abs(a - al))) / action_unit(kw))
    return worst


def g20_reference_error(pre):
    """(error of tanh(pre) against the fixture's mu, error of the actions against the fixture's relative to the action unit)."""
    (u, a), kw = g20_restated(pre)
    g = g20()
    return float(np.max(np.abs(np.tanh(u) - g[f"{pre}_mu"]))), float(np.max(np.abs(a - g[f"{pre}_action"]))) / action_unit(kw)
