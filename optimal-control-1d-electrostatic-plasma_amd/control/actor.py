"""The DeepSets particle actor a = pi(x, v) in the layout the device evaluates (pic_actor): the pooled particle
features of `BatchedPIC.pool` (the per-particle layer Linear(3, H) [-> LayerNorm] -> activation and the mean over the
particles), then a head of 1..6 linear layers with an optional LayerNorm and an activation behind every layer but the last, a
last linear layer and, with squash, a = action_shift + action_scale tanh(u).

The head's parameters are one flat float64 vector: per layer W [out][in] row-major, b [out] and -- with layernorm, behind every
layer but the last -- gamma [out], beta [out].  `BatchedPIC.actor_eval` and `BatchedPIC.step_actor` take a `ParticleActor`;
`from_reference` loads the state dict of an actor whose encoder is phi = Linear -> LayerNorm -> ReLU, the mean, rho = Linear ->
LayerNorm -> ReLU, followed by three Linear -> LayerNorm -> ReLU layers and a last Linear under a tanh; `to_torch` gives the
differentiable twin on (x, v) for env.grad.rollout_policy(observe="state"), `with_torch` repacks it after an update.  torch is
imported only by the methods that need it.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _head
from .._abi import ACTIVATIONS, PicActor, PicPoolLnSpec, PicPoolSpec
from ._head import _is_tensor

MAX_LAYERS, MAX_WIDTH = 6, 256

# what BatchedPIC.step_actor returns: features [T, E, H], pre (u) and actions (a) [T, E, 2M]; KE, PE, PE_reward [T, E] or None
ActorRollout = namedtuple("ActorRollout", "features pre actions KE PE PE_reward")


def head_param_count(widths, layernorm):
    """P: the length of one parameter vector of a head with these layer widths."""
    return _head.param_count(widths, layernorm)


def _host(a):
    """a (NumPy, a tensor or None) as a float64 NumPy array."""
    return _head._host(a, np.float64)


class ParticleActor:
    """The pool part: W [H, 3], b [H], optionally gamma and beta [H] of a LayerNorm(H, eps) inside the per-particle layer,
    `activation` ("tanh" or "relu") of the per-particle layer, v_scale, period (None or 0: the environment's L; with gamma and
    beta only).  The head: widths [H, ..., 2M] of 1..6 linear layers, params a flat float64 vector of
    `head_param_count(widths, layernorm)`, layernorm: a LayerNorm(width, ln_eps) behind every layer but the last,
    head_activation ("tanh" or "relu"; None: the pool's `activation`) behind every layer but the last; squash:
    a = action_shift + action_scale tanh(u) instead of a = u.  per_env: W, b (gamma, beta) carry a leading [num_envs] axis and
    params is [num_envs, P]."""

    def __init__(self, W, b, widths, params, activation="relu", gamma=None, beta=None, v_scale=1.0, eps=1e-5, period=None,
                 layernorm=False, ln_eps=1e-5, squash=False, action_scale=1.0, action_shift=0.0, per_env=False, head_activation=None):
        head_activation = activation if head_activation is None else head_activation
        for name, a in (("activation", activation), ("head_activation", head_activation)):
            if a not in ACTIVATIONS:
                raise ValueError(f"{name} must be one of {sorted(ACTIVATIONS)}, not {a!r}")
        self.activation, self.head_activation, self.per_env = activation, head_activation, bool(per_env)
        self.widths = [int(w) for w in widths]
        n = len(self.widths) - 1
        if not 1 <= n <= MAX_LAYERS:
            raise ValueError(f"a ParticleActor's head has 1..{MAX_LAYERS} linear layers, not {n}")
        if any(not 1 <= w <= MAX_WIDTH for w in self.widths):
            raise ValueError(f"every width must be 1..{MAX_WIDTH}: {self.widths}")
        lead = 1 if self.per_env else 0
        self.W, self.b, self.gamma, self.beta = _host(W), _host(b), _host(gamma), _host(beta)
        ws = self.W.shape
        if len(ws) != 2 + lead or ws[-1] != 3:
            raise ValueError(f"W must be {'[num_envs, H, 3]' if self.per_env else '[H, 3]'}, not {list(ws)}")
        H = ws[-2]
        if self.widths[0] != H:
            raise ValueError(f"the widths do not chain: the first is {self.widths[0]}, the pooled features have H = {H} entries")
        if (self.gamma is None) != (self.beta is None):
            raise ValueError("gamma and beta must both be given or both be None")
        for name, a in (("b", self.b), ("gamma", self.gamma), ("beta", self.beta)):
            if a is not None and a.shape != ws[:-1]:
                raise ValueError(f"{name} must have shape {list(ws[:-1])}, not {list(a.shape)}")
        self.v_scale, self.eps, self.period = float(v_scale), float(eps), (None if period is None else float(period))
        if not np.isfinite(self.v_scale):
            raise ValueError(f"v_scale must be finite, not {v_scale!r}")
        if self.gamma is not None:
            if not (np.isfinite(self.eps) and self.eps > 0):
                raise ValueError(f"eps must be finite and > 0, not {eps!r}")
            if self.period is not None and not (np.isfinite(self.period) and self.period >= 0):
                raise ValueError(f"period must be finite and >= 0 (0 or None: the environment's L), not {period!r}")
        self.layernorm, self.ln_eps = bool(layernorm), float(ln_eps)
        if self.layernorm and not (np.isfinite(self.ln_eps) and self.ln_eps > 0):
            raise ValueError(f"ln_eps must be finite and > 0, not {ln_eps!r}")
        self.squash, self.action_scale, self.action_shift = bool(squash), float(action_scale), float(action_shift)
        if not (np.isfinite(self.action_scale) and np.isfinite(self.action_shift)):
            raise ValueError("action_scale and action_shift must be finite")
        P = head_param_count(self.widths, self.layernorm)
        if not _is_tensor(params):
            params = np.ascontiguousarray(np.asarray(params, dtype=np.float64))
        shape = tuple(params.shape)
        if (len(shape) != 2 or shape[1] != P or shape[0] != ws[0]) if self.per_env else shape != (P,):
            raise ValueError(f"params must be {'[num_envs, P]' if self.per_env else '[P]'} with P = {P} for widths {self.widths}"
                             f"{' with layernorm' if self.layernorm else ''}, not {list(shape)}")
        self.params = params

    @property
    def hidden(self):
        return self.widths[0]

    @property
    def n_params(self):
        return head_param_count(self.widths, self.layernorm)

    # -- the flat vector <-> per-layer (W, b, gamma, beta) ---------------------------------------------------------------------
    @staticmethod
    def pack(layers):
        """[(W [out, in], b [out], gamma [out] or None, beta [out] or None), ...] -> the flat float64 vector; a tuple (W, b)
        stands for (W, b, None, None).  The layers must chain; with a LayerNorm every layer but the last has gamma and beta."""
        return _head.pack(layers)

    widths_of = staticmethod(_head.widths_of)

    def unpack(self, params=None):
        """The flat vector (this actor's, or one of its shape) -> [(W, b, gamma, beta), ...] as views (gamma, beta None where
        there is no LayerNorm); a [num_envs, P] array gives W [num_envs, out, in] and [num_envs, out] vectors."""
        return _head.unpack(self.params if params is None else params, self.widths, self.layernorm)

    def _kw(self):
        return dict(activation=self.activation, head_activation=self.head_activation, v_scale=self.v_scale, eps=self.eps, period=self.period, layernorm=self.layernorm,
                    ln_eps=self.ln_eps, squash=self.squash, action_scale=self.action_scale, action_shift=self.action_shift)

    def with_params(self, params=None, W=None, b=None, gamma=None, beta=None):
        """The same actor on another head vector and / or other tensors of the pool part (None: this actor's)."""
        pick = lambda new, old: old if new is None else new
        return ParticleActor(pick(W, self.W), pick(b, self.b), self.widths, pick(params, self.params), gamma=pick(gamma, self.gamma),
                             beta=pick(beta, self.beta), per_env=self.per_env, **self._kw())

    @classmethod
    def stack(cls, actors):
        """E actors of one shape -> one per-environment actor, environment e under actors[e]."""
        first = actors[0]
        key = lambda a: (a.widths, a.per_env, a.gamma is None, sorted(a._kw().items(), key=lambda kv: kv[0]))
        if first.per_env or any(key(a) != key(first) for a in actors):
            raise ValueError("stack: the actors must share their shape: widths, activation, the LayerNorms, scales and period")
        st = lambda name: None if getattr(first, name) is None else np.stack([getattr(a, name) for a in actors])
        return cls(st("W"), st("b"), first.widths, np.stack([_host(a.params) for a in actors]), gamma=st("gamma"), beta=st("beta"),
                   per_env=True, **first._kw())

    # -- the reference's actor -------------------------------------------------------------------------------------------------
    @classmethod
    def from_reference(cls, state_dict, L_ref=50.0, x_norm=1.0, v_norm=10.0, output_min=-1.0, output_max=1.0):
        """The actor of a DeepSets policy from its state dict (arrays or tensors, converted to float64): `encode.phi.0/1.*`
        (Linear(3, H) -> LayerNorm -> ReLU), the mean, `encode.rho.0/1.*`, `fc1`/`norm1` .. `fc3`/`norm3` (Linear -> LayerNorm
        -> ReLU each) and `fc_out` (or `fc_pi`) under a tanh that is rescaled to [output_min, output_max].  The network is fed
        x / x_norm and v / v_norm: period = L_ref x_norm, v_scale = 1 / v_norm, as PoolEncoder.from_reference."""
        get = lambda k: _host(state_dict[k])
        last = "fc_out" if "fc_out.weight" in state_dict else "fc_pi"
        layers = [(get("encode.rho.0.weight"), get("encode.rho.0.bias"), get("encode.rho.1.weight"), get("encode.rho.1.bias"))]
        layers += [(get(f"fc{i}.weight"), get(f"fc{i}.bias"), get(f"norm{i}.weight"), get(f"norm{i}.bias")) for i in (1, 2, 3)]
        layers.append((get(last + ".weight"), get(last + ".bias"), None, None))
        lo, hi = float(output_min), float(output_max)
        return cls(get("encode.phi.0.weight"), get("encode.phi.0.bias"), cls.widths_of(layers), cls.pack(layers), "relu",
                   gamma=get("encode.phi.1.weight"), beta=get("encode.phi.1.bias"), v_scale=1.0 / float(v_norm), eps=1e-5,
                   period=float(L_ref) * float(x_norm), layernorm=True, ln_eps=1e-5, squash=True, action_scale=(hi - lo) / 2,
                   action_shift=(hi + lo) / 2)

    # -- torch -----------------------------------------------------------------------------------------------------------------
    def to_torch(self, env, forward_ad=False):
        """The differentiable float64 twin on `env`: a module that maps the (x, v) of env.grad.rollout_policy(observe="state")
        to the actions without noise -- `pool` (control.pool.PoolEncoder: the library's pooled features as a torch op), then
        `head`, an nn.Sequential of Linear / LayerNorm / activation, then the squash.  Not for a per-environment actor."""
        import torch
        import torch.nn as nn
        from .pool import PoolEncoder
        if self.per_env:
            raise ValueError("to_torch: a per-environment actor has no single module (unpack() gives its weights)")
        actor = self

        class ActorTwin(nn.Module):
            def __init__(self):
                super().__init__()
                ln = actor.gamma is not None
                self.pool = PoolEncoder(env, actor.hidden, actor.activation, actor.v_scale, layernorm=ln, eps=actor.eps,
                                        period=actor.period or None, forward_ad=forward_ad)
                dev = self.pool.W.device
                with torch.no_grad():
                    for p, a in ((self.pool.W, actor.W), (self.pool.b, actor.b), (self.pool.gamma, actor.gamma), (self.pool.beta, actor.beta)):
                        if p is not None:
                            p.copy_(torch.from_numpy(np.ascontiguousarray(a)))
                self.head = nn.Sequential(*_head.torch_layers(actor.unpack(), actor.head_activation, actor.ln_eps)).to(dev)
                self.squash, self.action_scale, self.action_shift = actor.squash, actor.action_scale, actor.action_shift

            def forward(self, xv):
                u = self.head(self.pool(xv))
                return self.action_shift + self.action_scale * torch.tanh(u) if self.squash else u

        return ActorTwin()

    def with_torch(self, twin):
        """This actor on the parameters of `twin` (to_torch's module, e.g. after an optimiser step): the repacked actor."""
        import torch.nn as nn
        host = lambda p: None if p is None else p.detach().cpu().numpy()
        layers, mods = [], list(twin.head)
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                norm = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.LayerNorm) else None
                layers.append((host(m.weight), host(m.bias), host(norm.weight) if norm else None, host(norm.bias) if norm else None))
        pool = twin.pool
        return self.with_params(self.pack(layers), host(pool.W), host(pool.b), host(pool.gamma), host(pool.beta))

    # -- the C struct ----------------------------------------------------------------------------------------------------------
    def spec(self, mem, num_envs):
        """(PicActor, keep): the struct of a call in `mem`'s memory (env._arrays.Mem) and what its addresses point into (the pool's
        spec and parameters, the head's parameters), to be held until the call has read them."""
        if self.per_env and self.W.shape[0] != num_envs:
            raise ValueError(f"a per-environment actor needs parameters for {num_envs} environments, not {self.W.shape[0]}")
        H, ln = self.hidden, self.gamma is not None
        lead = (self.W.shape[0],) if self.per_env else ()
        parts = [self.W.reshape(lead + (3 * H,)), self.b] + ([self.gamma, self.beta] if ln else [])
        pool_params = mem.f64(np.ascontiguousarray(np.concatenate(parts, axis=-1)))
        act = ACTIVATIONS[self.activation]
        if ln:
            pool = PicPoolLnSpec(H, act, int(self.per_env), mem.kind, self.v_scale, self.eps, float(self.period or 0.0), mem.addr(pool_params))
        else:
            pool = PicPoolSpec(H, act, int(self.per_env), mem.kind, self.v_scale, mem.addr(pool_params))
        params = mem.f64(self.params)
        s = PicActor(None if ln else C.pointer(pool), C.pointer(pool) if ln else None, len(self.widths) - 1,
                     (C.c_int32 * 7)(*(self.widths + [0] * 7)[:7]), int(self.layernorm), ACTIVATIONS[self.head_activation], int(self.squash),
                     int(self.per_env),
                     self.ln_eps, self.action_scale, self.action_shift, mem.addr(params) or None)
        return s, (pool, pool_params, params)
