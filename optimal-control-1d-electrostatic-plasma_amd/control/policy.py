"""An MLP policy a = pi(o) on the Fourier modes of the mesh field, in the layout the device evaluates (pic_policy).

The parameters are one flat float64 vector: per layer W [out][in] row-major, then b [out].  `BatchedPIC.policy_eval` and
`BatchedPIC.step_policy` take an `MLPPolicy`; `from_torch` / `to_torch` move between it and an `nn.Sequential` for the update
step of a trainer.  torch is imported only by the methods that need it.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _head
from .._abi import ACTIVATIONS, PicPolicy
from ._head import _host, _is_tensor

MAX_LAYERS, MAX_WIDTH, MAX_OBS_MODES = 4, 256, 64

# what BatchedPIC.step_policy returns: obs [T, E, 2 M_o], pre (u) and actions (a) [T, E, 2M]; KE, PE, PE_reward [T, E] or None
PolicyRollout = namedtuple("PolicyRollout", "obs pre actions KE PE PE_reward")


def param_count(widths):
    """P: the length of one parameter vector of an MLP with these layer widths."""
    return _head.param_count(widths)


class MLPPolicy:
    """widths [2 M_o, ..., 2M] of 1..4 linear layers; activation "tanh" or "relu" behind every layer but the last; params a flat
    float64 vector of `param_count(widths)` (NumPy or a CUDA tensor), or [num_envs, P] with per_env; squash: a = action_scale *
    tanh(u) instead of a = u; obs_scale None or [2 M_o], multiplied into the observation before the first layer."""

    def __init__(self, widths, activation, params, obs_modes, squash=False, action_scale=1.0, obs_scale=None, per_env=False):
        self.widths = [int(w) for w in widths]
        self.obs_modes = int(obs_modes)
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, not {activation!r}")
        self.activation = activation
        n = len(self.widths) - 1
        if not 1 <= n <= MAX_LAYERS:
            raise ValueError(f"an MLPPolicy has 1..{MAX_LAYERS} linear layers, not {n}")
        if not 1 <= self.obs_modes <= MAX_OBS_MODES:
            raise ValueError(f"obs_modes must be 1..{MAX_OBS_MODES}, not {self.obs_modes}")
        if any(not 1 <= w <= MAX_WIDTH for w in self.widths):
            raise ValueError(f"every width must be 1..{MAX_WIDTH}: {self.widths}")
        if self.widths[0] != 2 * self.obs_modes:
            raise ValueError(f"the widths do not chain: the first is {self.widths[0]}, the observation has 2 obs_modes = "
                             f"{2 * self.obs_modes} entries")
        self.squash, self.action_scale, self.per_env = bool(squash), float(action_scale), bool(per_env)
        P = param_count(self.widths)
        if not _is_tensor(params):
            params = np.ascontiguousarray(np.asarray(params, dtype=np.float64))
        shape = tuple(params.shape)
        if (len(shape) != 2 or shape[1] != P) if self.per_env else shape != (P,):
            raise ValueError(f"params must be {'[num_envs, P]' if self.per_env else '[P]'} with P = {P} for widths {self.widths}, "
                             f"not {list(shape)}")
        self.params = params
        if obs_scale is not None:
            if not _is_tensor(obs_scale):
                obs_scale = np.ascontiguousarray(np.asarray(obs_scale, dtype=np.float64))
            if tuple(obs_scale.shape) != (self.widths[0],):
                raise ValueError(f"obs_scale must be [{self.widths[0]}], not {list(obs_scale.shape)}")
        self.obs_scale = obs_scale

    @property
    def n_params(self):
        return param_count(self.widths)

    # -- the flat vector <-> per-layer (W, b) ----------------------------------------------------------------------------------
    @staticmethod
    def pack(layers):
        """[(W [out, in], b [out]), ...] -> the flat float64 vector; the layers must chain (in of a layer = out of the one before)."""
        return _head.pack([(W, b) for W, b in layers])

    @staticmethod
    def widths_of(layers):
        return _head.widths_of([(W, b) for W, b in layers])

    def unpack(self, params=None):
        """The flat vector (this policy's, or one of its shape) -> [(W, b), ...] as views; a [num_envs, P] array gives
        W [num_envs, out, in] and b [num_envs, out]."""
        return [(W, b) for W, b, _, _ in _head.unpack(self.params if params is None else params, self.widths)]

    def unpack_grad(self, g):
        """A flat gradient with respect to the packed parameters ([P], or [num_envs, P]; NumPy or a tensor, e.g. what
        BatchedPIC.backward_policy or env.grad.rollout_mlp gives) -> [(gW [out, in], gb [out]), ...] with the layers' shapes, in
        the order of `to_torch()`'s Linear modules: the twin's optimiser takes them as .grad of weight and bias.  `pack` of the
        result is g again."""
        if tuple(np.shape(g))[-1:] != (self.n_params,):
            raise ValueError(f"a gradient of this policy ends in P = {self.n_params} entries, not {list(np.shape(g))}")
        return self.unpack(g)

    def pack_tangent(self, layers):
        """A direction in the parameters given as layers [(dW [out, in], db [out]), ...] (None for a part = zeros; e.g. the
        tangents of `to_torch()`'s Linear modules) -> the flat float64 vector [P] that BatchedPIC.policy_jvp / tangent_policy
        take as d_params; `unpack` of the result gives the layers again.  Stack K of them for K directions."""
        if len(layers) != len(self.widths) - 1:
            raise ValueError(f"a direction of this policy has {len(self.widths) - 1} layers, not {len(layers)}")
        full = []
        for l, (dW, db) in enumerate(layers):
            nin, nout = self.widths[l], self.widths[l + 1]
            dW = np.zeros((nout, nin)) if dW is None else np.asarray(_host(dW), dtype=np.float64)
            db = np.zeros(nout) if db is None else np.asarray(_host(db), dtype=np.float64)
            if dW.shape != (nout, nin) or db.shape != (nout,):
                raise ValueError(f"layer {l}: dW must be [{nout}, {nin}] and db [{nout}], not {dW.shape} and {db.shape}")
            full.append((dW, db))
        return self.pack(full)

    @classmethod
    def from_layers(cls, layers, activation, obs_modes, **kwargs):
        return cls(cls.widths_of(layers), activation, cls.pack(layers), obs_modes, **kwargs)

    # -- torch -----------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_torch(cls, module, obs_modes, action_scale=1.0, obs_scale=None):
        """An nn.Sequential of Linear layers with one kind of activation (Tanh or ReLU) between them and an optional final Tanh
        (squash) -> the packed policy; the weights are copied as float64."""
        import torch.nn as nn
        mods = list(module)
        squash = False
        if len(mods) > 1 and isinstance(mods[-1], nn.Tanh) and isinstance(mods[-2], nn.Linear):
            squash, mods = True, mods[:-1]
        layers, acts = [], set()
        for i, m in enumerate(mods):
            if i % 2 == 0:
                if not isinstance(m, nn.Linear) or m.bias is None:
                    raise ValueError(f"module {i} must be an nn.Linear with a bias, not {type(m).__name__}")
                layers.append((m.weight.detach().cpu().double().numpy(), m.bias.detach().cpu().double().numpy()))
            elif isinstance(m, nn.Tanh):
                acts.add("tanh")
            elif isinstance(m, nn.ReLU):
                acts.add("relu")
            else:
                raise ValueError(f"module {i} must be nn.Tanh or nn.ReLU, not {type(m).__name__}")
        if len(mods) % 2 == 0 or len(acts) > 1:
            raise ValueError("the module must be Linear (activation Linear)* [Tanh] with one kind of activation")
        return cls.from_layers(layers, acts.pop() if acts else "tanh", obs_modes, squash=squash, action_scale=action_scale,
                               obs_scale=obs_scale)

    def to_torch(self):
        """A float64 nn.Sequential with this policy's weights (a final Tanh with squash): u or tanh(u) of an observation that
        obs_scale has already been multiplied into; `torch_actions` applies both scales.  Not for a per-environment policy."""
        import torch.nn as nn
        if self.per_env:
            raise ValueError("to_torch: a per-environment policy has no single module (unpack() gives its weights)")
        mods = _head.torch_layers(_head.unpack(self.params, self.widths), self.activation)
        return nn.Sequential(*mods, *([nn.Tanh()] if self.squash else []))

    def torch_actions(self, module, obs):
        """The actions of `module` (to_torch's, or one of its shape) on observations obs [..., 2 M_o] with this policy's
        obs_scale and action_scale: the differentiable twin of the device's evaluation without noise."""
        import torch
        if self.obs_scale is not None:
            obs = obs * torch.as_tensor(self.obs_scale, dtype=obs.dtype, device=obs.device)
        out = module(obs)
        return self.action_scale * out if self.squash else out

    def with_params(self, params):
        """The same policy on another parameter vector (e.g. repacked after an update)."""
        return MLPPolicy(self.widths, self.activation, params, self.obs_modes, self.squash, self.action_scale, self.obs_scale,
                         self.per_env)

    @classmethod
    def stack(cls, policies):
        """E policies of one shape -> one per-environment policy, environment e under policies[e]."""
        first = policies[0]
        key = lambda p: (p.widths, p.activation, p.obs_modes, p.squash, p.action_scale, p.per_env)
        if first.per_env or any(key(p) != key(first) for p in policies):
            raise ValueError("stack: the policies must share widths, activation, obs_modes, squash and action_scale")
        scales = [_host(p.obs_scale) for p in policies]
        if any((s is None) != (scales[0] is None) or (s is not None and not np.array_equal(s, scales[0])) for s in scales):
            raise ValueError("stack: the policies must share obs_scale")
        flat = np.stack([_host(p.params) for p in policies])
        return cls(first.widths, first.activation, flat, first.obs_modes, first.squash, first.action_scale, first.obs_scale, True)

    # -- the C struct ----------------------------------------------------------------------------------------------------------
    def spec(self, mem, num_envs):
        """(PicPolicy, keep): the struct of a call in `mem`'s memory (env._arrays.Mem) and the arrays its addresses point into,
        to be held until the call has read them."""
        if self.per_env and self.params.shape[0] != num_envs:
            raise ValueError(f"a per-environment policy needs params [{num_envs}, P], not {list(self.params.shape)}")
        params, scale = mem.f64(self.params), mem.f64(self.obs_scale)
        width = (self.widths + [0] * 5)[:5]
        s = PicPolicy(self.obs_modes, len(self.widths) - 1, (C.c_int32 * 5)(*width), ACTIVATIONS[self.activation],
                      int(self.squash), int(self.per_env), self.action_scale, mem.addr(params) or None, mem.addr(scale) or None)
        return s, (params, scale)
