"""examples/policy_gradient.py's DeepSets policy with the per-particle layer and the mean computed by the library
(control.pool.PoolEncoder -> pic_pool / pic_pool_vjp): no [num_envs, N, hidden] tensor exists in the forward or in
the backward.  phi is one layer, tanh(W (cos q, sin q, v) + b), in float64; rho is the example's.  Trained with Adam on the same
cost on the same ensemble; prints J (mean over the ensemble) for each iteration.

    python examples/pooled_policy.py [num_envs] [N] [steps] [iterations] [--layernorm] [--jvp]

--jvp: instead of training, one directional derivative of the return along a random direction of the parameters, in forward
mode through env.grad.rollout_policy_jvp and the op's own tangent kernels (pic_pool_jvp), next to the same number
from the backward pass.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.control.pool import PoolEncoder  # noqa: E402
from policy_gradient import iteration  # noqa: E402


class PooledDeepSets(torch.nn.Module):
    """(x, v) [E, N] each -> actions [E, 2M]: PoolEncoder (phi and the mean, on the device's own kernels), then rho; the last
    layer starts at zero (a = 0: the uncontrolled plasma)."""

    def __init__(self, env, max_mode, hidden=32, layernorm=False, forward_ad=False):
        super().__init__()
        # --layernorm: phi = Linear -> LayerNorm -> ReLU, the reference encoder's per-particle layer (pic_pool_ln)
        self.enc = (PoolEncoder(env, hidden, "relu", layernorm=True, forward_ad=forward_ad) if layernorm
                    else PoolEncoder(env, hidden, forward_ad=forward_ad))
        self.rho = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2 * max_mode)).double()
        torch.nn.init.zeros_(self.rho[-1].weight)
        torch.nn.init.zeros_(self.rho[-1].bias)

    def forward(self, xv):
        return self.rho(self.enc(xv))


def make(env, max_mode, hidden=32, layernorm=False, forward_ad=False):
    torch.manual_seed(0)
    return PooledDeepSets(env, max_mode, hidden, layernorm, forward_ad).to("cuda")


def run(num_envs=64, N=5000, steps=50, iters=10, N_mesh=250, L=50.0, max_mode=5, lam=0.1, lr=0.02, seed=3, layernorm=False):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    policy = make(env, max_mode, layernorm=layernorm)
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        opt.zero_grad()
        J = iteration(env, policy, "state", steps, max_mode, lam, L, seed)
        opt.step()
        history.append(float(J.mean()))
        print(f"pooled  iter {it:2d}  J = {history[-1]:.6e}  ({time.perf_counter() - t0:.3f} s)", flush=True)
    env.stop_tape()
    env.close()
    return history


def run_jvp(num_envs=64, N=5000, steps=50, N_mesh=250, L=50.0, max_mode=5, lam=0.1, seed=3, layernorm=False):
    """dJ along one random direction of the parameters, J = sum over the ensemble of the training cost: forward mode against
    <grad J, direction> of the backward pass."""
    from ocplasma_amd.env import grad
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    policy = make(env, max_mode, layernorm=layernorm, forward_ad=True)
    with torch.no_grad():                                   # (the last layer starts at zero: move it, or every derivative is trivial)
        policy.rho[-1].weight.normal_(0.0, 0.1)
    params = dict(policy.named_parameters())
    g = torch.Generator().manual_seed(1)
    direction = {k: torch.randn(a.shape, generator=g, dtype=a.dtype).to(a.device) for k, a in params.items()}
    J = iteration(env, policy, "state", steps, max_mode, lam, L, seed)
    reverse = float(sum((a.grad * direction[k]).sum() for k, a in params.items()))
    env.stop_tape()
    env.reset_sampled("two-stream", seed=seed)
    fn = lambda q, o: torch.func.functional_call(policy, q, (o,))      # noqa: E731
    t0 = time.perf_counter()
    out = grad.rollout_policy_jvp(env, fn, {k: a.detach() for k, a in params.items()}, [direction], steps, observe="state")
    forward = float(out["dPE_reward"][0].sum() + 2.0 * lam * (out["actions"] * out["d_actions"][0]).sum() * L / 4)
    print(f"pooled  J = {float(J.sum()):.6e}  dJ forward mode {forward:.10e}  backward {reverse:.10e}  "
          f"({time.perf_counter() - t0:.3f} s for the tangent rollout)")
    env.stop_tape()
    env.close()
    return forward, reverse


if __name__ == "__main__":
    flags = ("--layernorm", "--jvp")
    sizes = [int(a) for a in sys.argv[1:] if a not in flags]
    if "--jvp" in sys.argv[1:]:
        run_jvp(*sizes[:3], layernorm="--layernorm" in sys.argv[1:])
    else:
        h = run(*sizes, layernorm="--layernorm" in sys.argv[1:])
        print(f"pooled: J {h[0]:.6e} -> {h[-1]:.6e}")
