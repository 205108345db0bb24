"""Pooled particle features as a torch op (pic_pool, pic_pool_vjp): the per-particle layer and the mean of a DeepSets
encoder on the particles themselves, phi(cos q, sin q, v) averaged over the particles, computed by the library without an
[num_envs, N, H] tensor in either pass.  `pooled_features` is differentiable with respect to x, v, W and b (reverse mode; with
forward_ad=True forward mode too: pic_pool_jvp), so a policy built on it plugs into
env.grad.rollout_policy(env, policy, T, observe="state") as any torch policy does, and with forward_ad=True into
env.grad.rollout_policy_jvp.

With gamma and beta the layer is Linear -> LayerNorm -> activation (pic_pool_ln, pic_pool_ln_vjp), differentiable
in gamma and beta too.  `PoolEncoder.from_reference` and `ReferenceEncoder` load the state dict of a DeepSets particle encoder
whose phi and rho are both Linear -> LayerNorm -> ReLU.
"""
import contextlib

import torch


class _Pooled(torch.autograd.Function):
    @staticmethod
    def forward(ctx, env, x, v, W, b, activation, v_scale):
        for name, t in (("x", x), ("v", v), ("W", W), ("b", b)):
            if not (t.is_cuda and t.dtype == torch.float64):
                raise ValueError(f"pooled_features: {name} must be a float64 CUDA tensor, not {t.dtype} on {t.device}")
        ctx.env, ctx.activation, ctx.v_scale = env, activation, float(v_scale)
        ctx.save_for_backward(x, v, W, b)
        return env.pool(W.detach(), b.detach(), activation, v_scale, x=x.detach(), v=v.detach(), on_device=True)

    @staticmethod
    def backward(ctx, cot):
        x, v, W, b = ctx.saved_tensors
        need = ctx.needs_input_grad                     # (env, x, v, W, b, activation, v_scale)
        g = ctx.env.pool_vjp(W, b, cot, ctx.activation, ctx.v_scale, x=x, v=v, on_device=True, g_x=need[1], g_v=need[2],
                             g_params=need[3] or need[4])
        return (None, g["g_x"], g["g_v"], g["g_W"] if need[3] else None, g["g_b"] if need[4] else None, None, None)


class _PooledLn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, env, x, v, W, b, gamma, beta, activation, v_scale, eps, period):
        for name, t in (("x", x), ("v", v), ("W", W), ("b", b), ("gamma", gamma), ("beta", beta)):
            if not (t.is_cuda and t.dtype == torch.float64):
                raise ValueError(f"pooled_features: {name} must be a float64 CUDA tensor, not {t.dtype} on {t.device}")
        ctx.env, ctx.kw = env, dict(activation=activation, v_scale=float(v_scale), eps=float(eps), period=period)
        ctx.save_for_backward(x, v, W, b, gamma, beta)
        return env.pool(W.detach(), b.detach(), x=x.detach(), v=v.detach(), on_device=True, gamma=gamma.detach(),
                        beta=beta.detach(), **ctx.kw)

    @staticmethod
    def backward(ctx, cot):
        x, v, W, b, gamma, beta = ctx.saved_tensors
        need = ctx.needs_input_grad                     # (env, x, v, W, b, gamma, beta, ...)
        g = ctx.env.pool_vjp(W, b, cot, x=x, v=v, on_device=True, g_x=need[1], g_v=need[2], g_params=any(need[3:7]), gamma=gamma,
                             beta=beta, **ctx.kw)
        grads = [g[k] if n else None for k, n in zip(("g_x", "g_v", "g_W", "g_b", "g_gamma", "g_beta"), need[1:7])]
        return (None, *grads, None, None, None, None)


def _plain(t):
    """A tensor that reaches a jvp, as the library can read it: without the wrappers of torch.func.jvp, which hands a jvp its
    saved tensors and tangents wrapped at the transform's level (they have no storage of their own).  Every level is taken off:
    what an outer transform (a jvp of the jvp, a vmap over the op) attached to the tensor is dropped."""
    f = getattr(torch._C, "_functorch", None)       # (a torch without torch.func has no wrappers)
    while f is not None and f.is_functorch_wrapped_tensor(t):
        t = f.get_unwrapped(t)
    return t


def _outside_transforms():
    """A context in which torch's ops on plain tensors give plain tensors: inside torch.func.jvp every op's result is wrapped at
    the transform's level, and pool_jvp builds the arrays it hands the library with torch's ops."""
    f = getattr(torch._C, "_functorch", None)
    if f is None:                                   # (a torch without torch.func: no transform can be active)
        return contextlib.nullcontext()
    try:
        from torch._functorch.pyfunctorch import temporarily_clear_interpreter_stack
    except ImportError as e:
        if f.get_dynamic_layer_stack_depth() == 0:  # (plain torch.autograd.forward_ad: nothing to step out of)
            return contextlib.nullcontext()
        raise RuntimeError("pooled_features(forward_ad=True): this torch has no torch._functorch.pyfunctorch."
                           "temporarily_clear_interpreter_stack, which the op's jvp needs under torch.func.jvp") from e
    return temporarily_clear_interpreter_stack()


def _tangents(tangents):
    """torch's tangents of a jvp as float64 tensors for pool_jvp (None = 0)."""
    return [None if t is None else _plain(t) for t in tangents]


class _PooledFwd(torch.autograd.Function):
    """_Pooled in the setup_context style, which torch.func.jvp and torch.autograd.forward_ad ask for, with a jvp."""

    @staticmethod
    def forward(env, x, v, W, b, activation, v_scale):
        for name, t in (("x", x), ("v", v), ("W", W), ("b", b)):
            if not (t.is_cuda and t.dtype == torch.float64):
                raise ValueError(f"pooled_features: {name} must be a float64 CUDA tensor, not {t.dtype} on {t.device}")
        return env.pool(W.detach(), b.detach(), activation, v_scale, x=x.detach(), v=v.detach(), on_device=True)

    @staticmethod
    def setup_context(ctx, inputs, output):
        env, x, v, W, b, activation, v_scale = inputs
        ctx.env, ctx.activation, ctx.v_scale = env, activation, float(v_scale)
        ctx.save_for_backward(x, v, W, b)
        ctx.save_for_forward(x, v, W, b)

    backward = staticmethod(_Pooled.backward)

    @staticmethod
    def jvp(ctx, _env, d_x, d_v, d_W, d_b, _activation, _v_scale):
        x, v, W, b = (_plain(t) for t in ctx.saved_tensors)
        d_x, d_v, d_W, d_b = _tangents((d_x, d_v, d_W, d_b))
        with _outside_transforms():
            return ctx.env.pool_jvp(W, b, d_x, d_v, d_W, d_b, ctx.activation, ctx.v_scale, x=x, v=v, on_device=True)


class _PooledLnFwd(torch.autograd.Function):
    """_PooledLn in the setup_context style, with a jvp."""

    @staticmethod
    def forward(env, x, v, W, b, gamma, beta, activation, v_scale, eps, period):
        for name, t in (("x", x), ("v", v), ("W", W), ("b", b), ("gamma", gamma), ("beta", beta)):
            if not (t.is_cuda and t.dtype == torch.float64):
                raise ValueError(f"pooled_features: {name} must be a float64 CUDA tensor, not {t.dtype} on {t.device}")
        return env.pool(W.detach(), b.detach(), activation, float(v_scale), x=x.detach(), v=v.detach(), on_device=True,
                        gamma=gamma.detach(), beta=beta.detach(), eps=float(eps), period=period)

    @staticmethod
    def setup_context(ctx, inputs, output):
        env, x, v, W, b, gamma, beta, activation, v_scale, eps, period = inputs
        ctx.env, ctx.kw = env, dict(activation=activation, v_scale=float(v_scale), eps=float(eps), period=period)
        ctx.save_for_backward(x, v, W, b, gamma, beta)
        ctx.save_for_forward(x, v, W, b, gamma, beta)

    backward = staticmethod(_PooledLn.backward)

    @staticmethod
    def jvp(ctx, _env, d_x, d_v, d_W, d_b, d_gamma, d_beta, *_):
        x, v, W, b, gamma, beta = (_plain(t) for t in ctx.saved_tensors)
        d_x, d_v, d_W, d_b, d_gamma, d_beta = _tangents((d_x, d_v, d_W, d_b, d_gamma, d_beta))
        with _outside_transforms():
            return ctx.env.pool_jvp(W, b, d_x, d_v, d_W, d_b, x=x, v=v, on_device=True, gamma=gamma, beta=beta, d_gamma=d_gamma,
                                    d_beta=d_beta, **ctx.kw)


def pooled_features(env, x, v, W, b, activation="tanh", v_scale=1.0, gamma=None, beta=None, eps=1e-5, period=None, forward_ad=False):
    """[num_envs, H]: out_k = mean_i act(b_k + W_k0 cos q_i + W_k1 sin q_i + W_k2 v_i v_scale), q = 2 pi x / L, of float64 CUDA
    tensors x, v [num_envs, N], W [H, 3] (or [num_envs, H, 3]) and b [H] (or [num_envs, H]) on `env` (a BatchedPIC), which
    supplies L, the stream and the working memory.  The backward is one pic_pool_vjp, which computes the gradients that are
    needed and no others.  By default forward mode is not built: torch raises its own error for a function without a jvp.
    With gamma and beta (shaped like b) a LayerNorm over the H units of each particle (eps) stands between the linear layer and
    the activation, and q = 2 pi x / period (None: the environment's L); differentiable in gamma and beta too.
    forward_ad=True: the same forward and backward, and forward mode as well -- under torch.autograd.forward_ad and
    torch.func.jvp (so under env.grad.rollout_policy_jvp) the tangent is one pic_pool_jvp call on the tangents torch hands over.
    One level of forward mode only: the jvp reads the data of its tensors, so a transform around it (torch.func.jvp of a jvp,
    vmap over the op) is silently not seen -- its tangents or batch dimension are dropped, not differentiated or mapped.
    It is a keyword, not the default, because it takes a second pair of autograd Functions in the setup_context style, which
    torch's forward mode insists on, and because the default op's behaviour under forward mode -- torch's own error -- is what
    callers and tests of the reverse-only op rely on."""
    if gamma is None and beta is None:
        return (_PooledFwd if forward_ad else _Pooled).apply(env, x, v, W, b, activation, v_scale)
    if gamma is None or beta is None:
        raise ValueError("pooled_features: gamma and beta must both be given or both be None")
    return (_PooledLnFwd if forward_ad else _PooledLn).apply(env, x, v, W, b, gamma, beta, activation, v_scale, eps, period)


class PoolEncoder(torch.nn.Module):
    """phi and the mean of a DeepSets encoder as one module: holds W [H, 3] and b [H] (float64) and maps the (x, v) tuple that
    rollout_policy(observe="state") hands a policy to the pooled features [num_envs, H].  With layernorm it also holds gamma
    (ones) and beta (zeros) [H] of a LayerNorm(H, eps) between the linear layer and the activation; `period` (None: the
    environment's L) is the period of the positions' features.  forward_ad: pooled_features' keyword (forward mode too)."""

    def __init__(self, env, hidden, activation="tanh", v_scale=1.0, scale=0.5, generator=None, layernorm=False, eps=1e-5, period=None,
                 forward_ad=False):
        super().__init__()
        if not 1 <= int(hidden) <= 256:
            raise ValueError(f"PoolEncoder: hidden must be 1..256, not {hidden}")
        dev = f"cuda:{env.device}"
        self.env, self.activation, self.v_scale = env, activation, float(v_scale)
        self.eps, self.period, self.forward_ad = float(eps), period, bool(forward_ad)
        r = lambda *s: torch.randn(*s, generator=generator, dtype=torch.float64)
        self.W = torch.nn.Parameter((r(int(hidden), 3) * scale).to(dev))
        self.b = torch.nn.Parameter((r(int(hidden)) * 0.1).to(dev))
        self.gamma = self.beta = None
        if layernorm:
            self.gamma = torch.nn.Parameter(torch.ones(int(hidden), dtype=torch.float64, device=dev))
            self.beta = torch.nn.Parameter(torch.zeros(int(hidden), dtype=torch.float64, device=dev))

    @classmethod
    def from_reference(cls, env, state_dict, L_ref=50.0, x_norm=1.0, v_norm=1.0, forward_ad=False):
        """The phi of a DeepSets particle encoder (Linear(3, H) -> LayerNorm(H) -> ReLU, period L_ref) from its state dict
        (`phi.0.weight`, `phi.0.bias`, `phi.1.weight`, `phi.1.bias`: arrays or tensors, converted to float64), for positions
        and velocities that the network is fed as x / x_norm and v / v_norm: period = L_ref x_norm, v_scale = 1 / v_norm."""
        get = lambda k: torch.as_tensor(state_dict[k]).detach().to(torch.float64)
        W = get("phi.0.weight")
        enc = cls(env, W.shape[0], "relu", 1.0 / float(v_norm), layernorm=True, eps=1e-5, period=float(L_ref) * float(x_norm),
                  forward_ad=forward_ad)
        with torch.no_grad():
            for p, k in ((enc.W, "phi.0.weight"), (enc.b, "phi.0.bias"), (enc.gamma, "phi.1.weight"), (enc.beta, "phi.1.bias")):
                p.copy_(get(k))
        return enc

    def forward(self, xv):
        x, v = xv
        return pooled_features(self.env, x, v, self.W, self.b, self.activation, self.v_scale, self.gamma, self.beta, self.eps, self.period,
                               self.forward_ad)


class ReferenceEncoder(torch.nn.Module):
    """A whole DeepSets particle encoder from its state dict: `PoolEncoder.from_reference` for phi and the mean, then rho =
    Linear(H, H_out) -> LayerNorm(H_out) -> ReLU as float64 torch layers (`rho.0.*`, `rho.1.*`).  Maps the (x, v) of
    rollout_policy(observe="state") to what the encoder returns for cat(x / x_norm, v / v_norm)."""

    def __init__(self, env, state_dict, L_ref=50.0, x_norm=1.0, v_norm=1.0, forward_ad=False):
        super().__init__()
        self.phi = PoolEncoder.from_reference(env, state_dict, L_ref, x_norm, v_norm, forward_ad)
        get = lambda k: torch.as_tensor(state_dict[k]).detach().to(torch.float64)
        Wr = get("rho.0.weight")
        lin, norm = torch.nn.Linear(Wr.shape[1], Wr.shape[0], dtype=torch.float64), torch.nn.LayerNorm(Wr.shape[0], eps=1e-5, dtype=torch.float64)
        with torch.no_grad():
            lin.weight.copy_(Wr)
            lin.bias.copy_(get("rho.0.bias"))
            norm.weight.copy_(get("rho.1.weight"))
            norm.bias.copy_(get("rho.1.bias"))
        self.rho = torch.nn.Sequential(lin, norm, torch.nn.ReLU()).to(self.phi.W.device)

    def forward(self, xv):
        return self.rho(self.phi(xv))
