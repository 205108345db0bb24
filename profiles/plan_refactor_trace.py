"""Launch geometry and HIP call sequence of a tree, for a parent-against-this-tree comparison (profiles/plan_refactor.md).

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/plan_refactor_trace.py geometry
  rocprofv3 --hip-trace    --output-format csv -d OUT -- python profiles/plan_refactor_trace.py calls

geometry: a handle and two steps (one call) for every bench.py configuration and for E = 4, N = 5000, Ng = 128 with blocks_per_env
0 (resident) and 3 (streaming).  placement="off": the search for a placement launches a number of probe kernels that follows the
clock, not the plan.  calls: the entry points whose read-back and staging code is shared, on the small shape in both schedules;
a hipDeviceSynchronize from here (the library never calls it) marks the start of each entry in the trace.
profiles/plan_refactor_compare.py compares two such output directories.  No torch in here: its calls would be in the trace."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd
from ocplasma_amd.env.batched import BatchedPIC

L = 50.0
SMALL = dict(num_envs=4, N=5000, N_mesh=128)


def geometry():
    configs = [dict(num_envs=1, N=10_000, N_mesh=128), dict(num_envs=64, N=1_000_000, N_mesh=256),
               dict(num_envs=128, N=1_000_000, N_mesh=512, dtype="float32", position_dtype="fixed32"),
               dict(num_envs=64, N=4_000_000, N_mesh=1024), dict(num_envs=128, N=10_000_000, N_mesh=256, dtype="float32"),
               dict(SMALL, blocks_per_env=0), dict(SMALL, blocks_per_env=3)]
    for c in configs:
        env = BatchedPIC(L=L, dt=0.1, placement="off", **c)
        env.reset_sampled("bump-on-tail", seed=1)
        env.step(None, 2)
        env.sync()
        print(c, env._h.schedule(), flush=True)
        env.close()


def calls():
    hip = ctypes.CDLL("libamdhip64.so")
    rng = np.random.default_rng(0)
    E, N, Ng = SMALL["num_envs"], SMALL["N"], SMALL["N_mesh"]
    for bpe in (0, 3):
        env = BatchedPIC(L=L, dt=0.1, blocks_per_env=bpe, **SMALL)
        env.reset_sampled("bump-on-tail", seed=1)
        env.set_actuator(ocplasma_amd.E_field(L, Ng, 2))
        env.step(None, 1)
        env.sync()
        x = rng.uniform(0, L, (E, N))
        ext = rng.normal(size=(E, Ng))
        h = env._h
        entries = [("pic_get_fields", env.fields), ("pic_get_energies", env.energies), ("pic_get_particles", env.particles),
                   ("pic_eval_field (small host state)", lambda: env.eval_field(x, ext)),
                   ("pic_compute_E", lambda: h.compute_E(x, ext, particles=True, shape=True)),
                   ("pic_solve_poisson", lambda: h.solve_poisson(ext - ext.mean(axis=1, keepdims=True))),
                   ("pic_get_modes", lambda: env.modes(2)), ("pic_step_observe (E_ext)", lambda: env.step_observe(E_external=ext)),
                   ("pic_step_observe (2 steps)", lambda: env.step_observe(nsteps=2)),
                   ("pic_step_ext_traj", lambda: env.step_ext_traj(np.stack([ext, ext]), history=True)),
                   ("pic_step_feedback_gain (host gain)", lambda: env.step_feedback_gain(np.eye(4), 2, actions=True, modes=True))]
        for name, f in entries:
            hip.hipDeviceSynchronize()
            f()
            print(bpe, name, flush=True)
        hip.hipDeviceSynchronize()
        env.close()
    # pic_eval_field's other path: a host state too large for the pinned staging
    env = BatchedPIC(64, 20000, 128, L=L, dt=0.1)
    env.reset_sampled("bump-on-tail", seed=1)
    hip.hipDeviceSynchronize()
    env.eval_field(rng.uniform(0, L, (64, 20000)))
    print("pic_eval_field (scratch path)", flush=True)
    hip.hipDeviceSynchronize()
    env.close()


if __name__ == "__main__":
    {"geometry": geometry, "calls": calls}[sys.argv[1]]()
