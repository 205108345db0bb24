"""Pooled particle features as a torch op (pic_pool, pic_pool_vjp): the per-particle layer and the mean of a DeepSets
encoder on the particles themselves, phi(cos q, sin q, v) averaged over the particles, computed by the library without an
[num_envs, N, H] tensor in either pass.  `pooled_features` is differentiable with respect to x, v, W and b (reverse mode only),
so a policy built on it plugs into env.grad.rollout_policy(env, policy, T, observe="state") as any torch policy does.
"""
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


def pooled_features(env, x, v, W, b, activation="tanh", v_scale=1.0):
    """[num_envs, H]: out_k = mean_i act(b_k + W_k0 cos q_i + W_k1 sin q_i + W_k2 v_i v_scale), q = 2 pi x / L, of float64 CUDA
    tensors x, v [num_envs, N], W [H, 3] (or [num_envs, H, 3]) and b [H] (or [num_envs, H]) on `env` (a BatchedPIC), which
    supplies L, the stream and the working memory.  The backward is one pic_pool_vjp, which computes the gradients that are
    needed and no others.  Forward mode is not built: torch raises its own error for a function without a jvp."""
    return _Pooled.apply(env, x, v, W, b, activation, v_scale)


class PoolEncoder(torch.nn.Module):
    """phi and the mean of a DeepSets encoder as one module: holds W [H, 3] and b [H] (float64) and maps the (x, v) tuple that
    rollout_policy(observe="state") hands a policy to the pooled features [num_envs, H]."""

    def __init__(self, env, hidden, activation="tanh", v_scale=1.0, scale=0.5, generator=None):
        super().__init__()
        if not 1 <= int(hidden) <= 256:
            raise ValueError(f"PoolEncoder: hidden must be 1..256, not {hidden}")
        dev = f"cuda:{env.device}"
        self.env, self.activation, self.v_scale = env, activation, float(v_scale)
        r = lambda *s: torch.randn(*s, generator=generator, dtype=torch.float64)
        self.W = torch.nn.Parameter((r(int(hidden), 3) * scale).to(dev))
        self.b = torch.nn.Parameter((r(int(hidden)) * 0.1).to(dev))

    def forward(self, xv):
        x, v = xv
        return pooled_features(self.env, x, v, self.W, self.b, self.activation, self.v_scale)
