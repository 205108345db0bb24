"""HIP call sequence and kernel launches of the two controllers' entries, for a parent-against-this-tree comparison
(profiles/head_refactor.md), in the manner of profiles/plan_refactor_trace.py:

  rocprofv3 --hip-trace --kernel-trace --output-format csv -d OUT -- python profiles/head_refactor_trace.py

On the smallest shape the GPU tests use (two environments, 48 particles, a 16-point mesh, one actuator mode): create, reset,
set_actuator, then pic_policy_eval, pic_policy_vjp, pic_policy_jvp, pic_step_policy (3 steps), pic_tape_step_policy (3 steps on
an open tape), pic_actor_eval on given features and on the stored particles, and pic_step_actor (3 steps) under a plain and a
LayerNorm pool -- each once in host memory and once in device memory, with noise, std, every output and the energies' record.  A
hipDeviceSynchronize from here (the library never calls it) marks the start of each entry in the trace;
profiles/plan_refactor_compare.py compares two such output directories section by section.  torch carries the arrays of the
device-memory calls: its own HIP calls are in both traces alike, and its start-up is in the set-up section."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd
from ocplasma_amd.control.actor import ParticleActor, head_param_count
from ocplasma_amd.control.policy import MLPPolicy, param_count
from ocplasma_amd.env.batched import BatchedPIC

E, N, NG, M, MO, H, T, L = 2, 48, 16, 1, 1, 5, 3, 50.0


def main():
    import torch
    hip = ctypes.CDLL("libamdhip64.so")
    rng = np.random.default_rng(0)
    env = BatchedPIC(E, N, NG, L=L, dt=0.1)
    env.reset_sampled("two-stream", seed=1)
    env.set_actuator(ocplasma_amd.E_field(L, NG, M))
    torch.zeros(1, dtype=torch.float64, device="cuda").add_(1.0)
    torch.cuda.synchronize()
    widths = [2 * MO, 5, 2 * M]
    pol = MLPPolicy(widths, "tanh", 0.3 * rng.standard_normal(param_count(widths)), MO, squash=True, action_scale=0.5,
                    obs_scale=np.full(2 * MO, 4.0))
    head = [H, 7, 2 * M]
    actors = {}
    for name, ln in (("pool", {}), ("pool_ln", dict(gamma=rng.uniform(0.5, 1.5, H), beta=rng.uniform(-0.5, 0.5, H)))):
        actors[name] = ParticleActor(0.5 * rng.normal(size=(H, 3)), 0.1 * rng.normal(size=H), head,
                                     0.3 * rng.standard_normal(head_param_count(head, True)), "relu", v_scale=0.1, layernorm=True,
                                     squash=True, action_scale=0.5, **ln)
    obs, pre, cot = rng.normal(size=(E, 2 * MO)), rng.normal(size=(E, 2 * M)), rng.normal(size=(E, 2 * M))
    d_params, feats = rng.normal(size=param_count(widths)), rng.normal(size=(E, H))
    eps1, epsT, std = rng.normal(size=(E, 2 * M)), rng.normal(size=(T, E, 2 * M)), np.full(2 * M, 0.1)

    def taped(dev):
        env.start_tape(2 * T)
        env.tape_step_policy(pol, T, noise=epsT, std=std, on_device=dev)
        env.stop_tape()
    for dev in (False, True):
        entries = [("pic_policy_eval", lambda: env.policy_eval(pol, noise=eps1, std=std, on_device=dev)),
                   ("pic_policy_eval (obs)", lambda: env.policy_eval(pol, obs=obs, on_device=dev)),
                   ("pic_policy_vjp", lambda: env.policy_vjp(pol, obs, cot, pre, on_device=dev)),
                   ("pic_policy_jvp", lambda: env.policy_jvp(pol, obs, pre, d_params=d_params, d_obs=obs, on_device=dev)),
                   ("pic_step_policy", lambda: env.step_policy(pol, T, noise=epsT, std=std, on_device=dev)),
                   ("pic_tape_step_policy", lambda: taped(dev)),
                   ("pic_actor_eval (features)", lambda: env.actor_eval(actors["pool"], features=feats, noise=eps1, std=std, on_device=dev)),
                   ("pic_actor_eval (particles)", lambda: env.actor_eval(actors["pool"], noise=eps1, std=std, on_device=dev)),
                   ("pic_actor_eval (particles, pool_ln)", lambda: env.actor_eval(actors["pool_ln"], on_device=dev)),
                   ("pic_step_actor (pool)", lambda: env.step_actor(actors["pool"], T, noise=epsT, std=std, on_device=dev)),
                   ("pic_step_actor (pool_ln)", lambda: env.step_actor(actors["pool_ln"], T, noise=epsT, std=std, on_device=dev))]
        for name, f in entries:
            hip.hipDeviceSynchronize()
            f()
            print("device" if dev else "host", name, flush=True)
    hip.hipDeviceSynchronize()
    assert env.bad_count() == 0
    env.close()


if __name__ == "__main__":
    main()
