"""Forward-mode sensitivities of a taped rollout (pic_tape_tangent): the Jacobian of the PE_reward trace with
respect to the 2M coefficients of a constant action, all K = 2M directions in ONE call, printed next to central differences of
the device's own rollouts.  This is the Jacobian a Gauss-Newton or Levenberg-Marquardt step on the reference's cost (a sum of
squares of field values) needs; reverse mode would need one backward per step of the trace.

    python examples/tangent_sensitivity.py [num_envs] [N] [steps] [max_mode]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402


def run(num_envs=2, N=20000, steps=20, max_mode=3, N_mesh=128, L=50.0, eps=1e-6, seed=3):
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    n = 2 * max_mode
    a0 = np.random.default_rng(seed).uniform(-0.3, 0.3, (num_envs, n))
    held = np.broadcast_to(a0, (steps, num_envs, n)).copy()              # the same action at every step
    env.reset_sampled("bump-on-tail", seed=seed)
    env.sync()
    x0, v0 = env.particles()
    env.start_tape(steps)
    env.step_actions_traj(held)
    # direction k: d a_t = unit vector k at every step, in every environment
    da = np.zeros((n, steps, num_envs, n))
    for k in range(n):
        da[k, :, :, k] = 1.0
    jac = env.tangent(d_actions=da)["PE_reward"]                        # [2M, T, num_envs]: d PE_reward_t / d a_k
    env.stop_tape()
    fd = np.empty_like(jac)
    for k in range(n):
        pers = []
        for sgn in (1.0, -1.0):
            env.reset(x0, v0)
            _, _, per = env.step_actions_traj(held + sgn * eps * da[k], history=True)
            pers.append(per)
        fd[k] = (pers[0] - pers[1]) / (2 * eps)
    env.close()
    for e in range(num_envs):
        print(f"environment {e}: d PE_reward_t / d a_k at the last step, forward mode vs central differences (eps = {eps:g})")
        for k in range(n):
            print(f"  a_{k}: {jac[k, -1, e]: .10e}  {fd[k, -1, e]: .10e}")
    rel = float(np.max(np.abs(jac - fd)) / np.max(np.abs(jac)))
    print(f"max |J - FD| / max |J| over the whole trace: {rel:.2e}")
    return jac, fd


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:5]]
    run(*args)
