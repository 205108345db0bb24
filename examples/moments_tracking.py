"""Tracking a density profile with open-loop actions by Gauss-Newton steps.

The cost is J(a) = sum_t |m0_t(a) - target|^2 over the densities m0_t [num_envs, N_mesh] of the states a rollout under the
actions a [T, num_envs, 2M] leaves.  With the residual r = m0 - target and the Jacobian Jac = d m0 / d a, a Gauss-Newton step
solves (Jac^T Jac + mu) p = -Jac^T r by a few iterations of conjugate gradients.  Both products come from the same tape:

    Jac u    = env.tangent(moments=True, d_actions=u)["moments"][:, :, 0]        (pic_tape_tangent_moments, forward mode)
    Jac^T w  = env.backward(d_moments=rows(w))["actions"]                         (pic_tape_moments_cot, reverse mode)

so one rollout serves the whole step, and the slope of J along p, 2 <r, Jac p>, is known before p is tried.  Prints J for each
iteration; it goes down.

    python examples/moments_tracking.py [num_envs] [N] [steps] [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field  # noqa: E402


def main():
    E, N, T, iters = (int(a) for a in (sys.argv[1:5] + ["4", "20000", "10", "4"][len(sys.argv) - 1:]))
    Ng, M, L = 64, 3, 50.0
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1)
    env.set_actuator(E_field(L, Ng, M))
    target = 1.0 + 0.02 * np.cos(2 * np.pi * np.arange(Ng) / Ng)         # a standing density wave in mode 1

    def rollout(a):
        """A fresh tape with the moments' trace under a; returns the residual [T, E, Ng]."""
        env.stop_tape()
        env.reset_sampled("bump-on-tail", seed=1)
        env.start_tape(T, moments=True)
        env.step_actions_traj(a)
        return env.tape_moments()[:, :, 0] - target

    def rows(w):
        c = np.zeros((T, E, 3, Ng))
        c[:, :, 0] = w
        return c

    jac = lambda u: env.tangent(moments=True, d_actions=u)["moments"][:, :, 0]      # noqa: E731
    jac_t = lambda w: env.backward(d_moments=rows(w))["actions"]                    # noqa: E731

    a = np.zeros((T, E, 2 * M))
    r = rollout(a)
    mu = 1e-6
    for it in range(iters):
        cost = float((r * r).sum())
        g = jac_t(r)                                        # half the gradient of J
        # conjugate gradients on (Jac^T Jac + mu) p = -g
        p, res = np.zeros_like(a), -g
        d, rs = res.copy(), float((res * res).sum())
        for _ in range(5):
            Jd = jac(d)
            Ad = jac_t(Jd) + mu * d
            alpha = rs / float((d * Ad).sum())
            p, res = p + alpha * d, res - alpha * Ad
            rs_new = float((res * res).sum())
            if rs_new < 1e-20 * float((g * g).sum()):
                break
            d, rs = res + (rs_new / rs) * d, rs_new
        slope = 2.0 * float((r * jac(p)).sum())             # dJ/dstep at 0 along p, before p is tried
        step = 1.0
        while True:                                         # halve the step until the cost goes down
            r_new = rollout(a + step * p)
            if float((r_new * r_new).sum()) < cost or step < 1e-3:
                break
            step *= 0.5
        a, r = a + step * p, r_new
        print(f"iteration {it}: J = {cost:.6e} -> {float((r * r).sum()):.6e}   slope along p = {slope:.3e}   step = {step:g}")
    env.stop_tape()
    env.close()


if __name__ == "__main__":
    main()
