"""Eight parameter directions of a closed-loop rollout's cost in ONE forward-mode pass on the device (BatchedPIC.tangent_policy ->
pic_tape_tangent_policy), checked against the reverse pass on the same tape by duality.

An ensemble of two-stream environments runs T steps under an MLP policy on the Fourier modes of the field (tape_step_policy).  For
the reference's cost, summed over the rollout and the ensemble,

    J = sum_t PE_reward_t + lam * sum_t |a_t|^2 L / 4,

the directional derivatives dJ[k] = <dJ/dtheta, d_k> along K = 8 random directions d_k in the packed parameters come out of one
tangent_policy call: dJ[k] = sum dPE_reward[k] + lam L / 2 * sum a * d_actions[k].  One backward_policy on the same tape gives
the whole gradient; <gradient, d_k> must agree with dJ[k] to rounding.  The second half is what forward mode is for: a
Gauss-Newton product J_a^T J_a d of the actions' Jacobian, one tangent_policy followed by one backward_policy.

    python examples/policy_sensitivity_device.py [num_envs] [N] [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402
from ocplasma_amd.control.policy import MLPPolicy, param_count  # noqa: E402


def run(num_envs=64, N=5000, steps=50, N_mesh=250, L=50.0, max_mode=3, obs_modes=3, hidden=64, lam=0.1, K=8, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.use_torch_stream()
    f64 = dict(dtype=torch.float64, device="cuda")
    widths = [2 * obs_modes, hidden, hidden, 2 * max_mode]
    rng = np.random.default_rng(seed)
    policy = MLPPolicy(widths, "tanh", torch.tensor(0.3 * rng.standard_normal(param_count(widths)), **f64), obs_modes,
                       obs_scale=torch.full((2 * obs_modes,), 8.0, **f64))
    directions = torch.tensor(rng.standard_normal((K, policy.n_params)), **f64)

    env.reset_sampled("two-stream", seed=seed)
    env.start_tape(steps)
    r = env.tape_step_policy(policy, steps, on_device=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tan = env.tangent_policy(d_params=directions)                       # K directions, one pass
    torch.cuda.synchronize()
    t_fwd = time.perf_counter() - t0
    dJ = tan["dPE_reward"].sum(dim=(1, 2)) + lam * L / 2 * (r.actions[None] * tan["d_actions"]).sum(dim=(1, 2, 3))

    t0 = time.perf_counter()
    ones = torch.ones((steps, num_envs), **f64)
    g = env.backward_policy(d_PE_reward=ones, d_actions=lam * L / 2 * r.actions)   # the whole gradient, one pass
    torch.cuda.synchronize()
    t_bwd = time.perf_counter() - t0
    dual = directions @ g["params"]
    gap = float(((dJ - dual).abs() / torch.maximum(dJ.abs(), dual.abs())).max())
    for k in range(K):
        print(f"direction {k}: dJ forward {float(dJ[k]): .10e}   <grad, d> {float(dual[k]): .10e}")
    print(f"largest relative gap {gap:.2e};  tangent_policy ({K} directions) {1e3 * t_fwd:.1f} ms, backward_policy {1e3 * t_bwd:.1f} ms")
    assert gap < 1e-9, gap

    # a Gauss-Newton product of the actions' Jacobian J_a = d actions / d theta:  J_a^T (J_a d_0)
    ja_d = env.tangent_policy(d_params=directions[0])["d_actions"]
    gn = env.backward_policy(d_actions=ja_d)["params"]
    print(f"Gauss-Newton: d^T J_a^T J_a d = {float(directions[0] @ gn):.10e}   |J_a d|^2 = {float((ja_d ** 2).sum()):.10e}")
    assert abs(float(directions[0] @ gn) - float((ja_d ** 2).sum())) <= 1e-9 * float((ja_d ** 2).sum())
    env.stop_tape()
    env.close()
    return gap


if __name__ == "__main__":
    run(*[int(a) for a in sys.argv[1:]])
