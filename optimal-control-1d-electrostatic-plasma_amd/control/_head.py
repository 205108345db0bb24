"""What `MLPPolicy` (control/policy.py) and the head of `ParticleActor` (control/actor.py) share: one flat float64 parameter
vector -- per layer W [out][in] row-major, b [out] and, with a LayerNorm behind every layer but the last, gamma [out], beta
[out] -- and its per-layer form [(W, b, gamma, beta), ...] (gamma, beta None where there is no LayerNorm; a pair (W, b) stands
for (W, b, None, None)).  torch is imported only by `torch_layers`.
"""
import numpy as np


def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _host(a, dtype=None):
    """a (NumPy, a tensor or None) as a NumPy array, of `dtype` if one is given."""
    return None if a is None else np.asarray(a.detach().cpu().numpy() if _is_tensor(a) else a, dtype=dtype)


def param_count(widths, layernorm=False):
    """P: the length of one parameter vector for these layer widths."""
    n = len(widths) - 1
    return sum(widths[l + 1] * widths[l] + widths[l + 1] + (2 * widths[l + 1] if layernorm and l + 1 < n else 0) for l in range(n))


def pack(layers):
    """The per-layer form -> the flat float64 vector.  The layers must chain (in of a layer = out of the one before); with a
    LayerNorm every layer but the last has gamma and beta."""
    parts, prev = [], None
    norms = [len(t) == 4 and t[2] is not None for t in layers]
    if norms[-1] or len(set(norms[:-1])) > 1:
        raise ValueError("pack: gamma and beta belong behind every layer but the last, or behind none")
    for l, t in enumerate(layers):
        W, b = np.asarray(t[0], dtype=np.float64), np.asarray(t[1], dtype=np.float64)
        if W.ndim != 2 or b.shape != (W.shape[0],):
            raise ValueError(f"layer {l}: W must be [out, in] and b [out], not {W.shape} and {b.shape}")
        if prev is not None and W.shape[1] != prev:
            raise ValueError(f"the widths do not chain: layer {l} takes {W.shape[1]} inputs, layer {l - 1} gives {prev}")
        prev = W.shape[0]
        parts += [W.ravel(), b]
        if norms[l]:
            g, be = np.asarray(t[2], dtype=np.float64), np.asarray(t[3], dtype=np.float64)
            if g.shape != b.shape or be.shape != b.shape:
                raise ValueError(f"layer {l}: gamma and beta must be [{prev}], not {g.shape} and {be.shape}")
            parts += [g, be]
    return np.concatenate(parts)


def widths_of(layers):
    return [int(np.shape(layers[0][0])[1])] + [int(np.shape(t[0])[0]) for t in layers]


def unpack(params, widths, layernorm=False):
    """A flat vector for these widths (NumPy or a tensor) -> the per-layer form as float64 views; a [num_envs, P] array gives
    W [num_envs, out, in] and [num_envs, out] vectors."""
    p = _host(params, np.float64)
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
    return out


def torch_layers(layers, activation, ln_eps=1e-5):
    """The float64 torch modules of the per-layer form: Linear [-> LayerNorm(out, ln_eps)] -> Tanh or ReLU for every layer but
    the last, then the last Linear."""
    import torch
    import torch.nn as nn

    def filled(mod, weight, bias):
        with torch.no_grad():
            mod.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight)))
            mod.bias.copy_(torch.from_numpy(np.ascontiguousarray(bias)))
        return mod
    mods = []
    for l, (W, b, g, be) in enumerate(layers):
        mods.append(filled(nn.Linear(W.shape[1], W.shape[0], dtype=torch.float64), W, b))
        if l + 1 == len(layers):
            break
        if g is not None:
            mods.append(filled(nn.LayerNorm(W.shape[0], eps=ln_eps, dtype=torch.float64), g, be))
        mods.append(nn.Tanh() if activation == "tanh" else nn.ReLU())
    return mods
