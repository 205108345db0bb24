"""Forward-mode sensitivities of a taped rollout (pic_tape_tangent): the Jacobian of the PE_reward trace with
respect to the 2M coefficients of a constant action, all K = 2M directions in ONE call, printed next to central differences of
the device's own rollouts.  This is the Jacobian a Gauss-Newton or Levenberg-Marquardt step on the reference's cost (a sum of
squares of field values) needs; reverse mode would need one backward per step of the trace.  The tape also records the smoothed
phase-space KL against the starting state, and the same call returns its tangents (pic_tape_tangent_kl, 7j): the
directional derivatives of the whole cost sum_t (KL~_t + PE_reward_t) along the 2M directions, which a line search on it needs.

    python examples/tangent_sensitivity.py [num_envs] [N] [steps] [max_mode]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402


def run(num_envs=2, N=20000, steps=20, max_mode=3, N_mesh=128, L=50.0, eps=1e-6, eps_cost=1e-4, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    n = 2 * max_mode
    a0 = np.random.default_rng(seed).uniform(-0.3, 0.3, (num_envs, n))
    held = np.broadcast_to(a0, (steps, num_envs, n)).copy()              # the same action at every step
    env.reset_sampled("bump-on-tail", seed=seed)
    env.sync()
    x0, v0 = env.particles()
    kl = dict(feq=env.phase_density_smooth(32, -6.0, 6.0), vmin=-6.0, vmax=6.0)     # the target: the starting state's density
    env.start_tape(steps, kl=kl)
    env.step_actions_traj(held)
    # direction k: d a_t = unit vector k at every step, in every environment
    da = np.zeros((n, steps, num_envs, n))
    for k in range(n):
        da[k, :, :, k] = 1.0
    tan = env.tangent(d_actions=da, kl=True)
    jac = tan["PE_reward"]                                              # [2M, T, num_envs]: d PE_reward_t / d a_k
    dcost = (tan["KL"] + tan["PE_reward"]).sum(axis=1)                  # [2M, num_envs]: d sum_t (KL~_t + PE_reward_t) / d a_k
    env.stop_tape()
    fd, fd_cost = np.empty_like(jac), np.empty_like(dcost)
    # The KL~ comes from integer weights (2^-24 of a particle per axis at N = 20000): a difference quotient of it carries that
    # rounding divided by the step, so the cost is differenced with the larger step eps_cost.
    for k in range(n):
        pers, costs = [], []
        for step in (eps, eps_cost):
            for sgn in (1.0, -1.0):
                env.reset(x0, v0)
                env.start_tape(steps, kl=kl)
                _, _, per = env.step_actions_traj(held + sgn * step * da[k], history=True)
                if step == eps:
                    pers.append(per)
                else:
                    costs.append((env.tape_kl() + per).sum(axis=0))
                env.stop_tape()
        fd[k] = (pers[0] - pers[1]) / (2 * eps)
        fd_cost[k] = (costs[0] - costs[1]) / (2 * eps_cost)
    env.close()
    for e in range(num_envs):
        print(f"environment {e}: d PE_reward_t / d a_k at the last step, forward mode vs central differences (eps = {eps:g})")
        for k in range(n):
            print(f"  a_{k}: {jac[k, -1, e]: .10e}  {fd[k, -1, e]: .10e}")
    rel = float(np.max(np.abs(jac - fd)) / np.max(np.abs(jac)))
    print(f"max |J - FD| / max |J| over the whole trace: {rel:.2e}")
    for e in range(num_envs):
        print(f"environment {e}: d sum_t (KL~_t + PE_reward_t) / d a_k, forward mode vs central differences (eps = {eps_cost:g})")
        for k in range(n):
            print(f"  a_{k}: {dcost[k, e]: .10e}  {fd_cost[k, e]: .10e}")
    print("(the KL~ is a sum of integer weights: its difference quotient is exact only down to their rounding divided by eps, "
          "a few 1e-5 relative here; the forward-mode value is the derivative of the unrounded weights)")
    return jac, fd


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:5]]
    run(*args)
