"""Look at a rollout without a particle snapshot: the feedback controller of examples/feedback_control.py on a batch of
two-stream environments with the recorder on (BatchedPIC.recording -> pic_record_*).  Every `stride`-th step the device
reduces each environment's state to its energies, field energy, Fourier spectrum, x / v histograms and the entropy and KL
cost of its phase-space density; the records are read back once at the end and saved as .npz.

    python examples/record_rollout.py [num_envs] [N] [steps] [stride] [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ocplasma_amd  # noqa: F401,E402
from ocplasma_amd import BatchedPIC, E_field, TwoStream  # noqa: E402
from ocplasma_amd.interpret import landau  # noqa: E402


def run(num_envs=4, N=20000, steps=300, stride=2, out="record_rollout.npz", N_mesh=128, L=50.0, max_mode=5, seed=11,
        phase_bins=64, vmin=-10.0, vmax=10.0, t_linear=(2.0, 12.0)):
    np.random.seed(seed)
    dist = TwoStream(v0=3.0, sigma=1.0, n_samples=N, L=L)
    xs, vs = [], []
    for _ in range(num_envs):
        dist.reinit()
        x, v = dist.get_sample()
        xs.append(x)
        vs.append(v * (1 + 0.1 * np.sin(2 * np.pi * 2 * x / L)))     # PIC.initialize perturbation, n_mode = 2
    env = BatchedPIC(num_envs, N, N_mesh, L=L, dt=0.1)
    env.set_actuator(E_field(L, N_mesh, max_mode))
    env.reset(np.stack(xs), np.stack(vs))
    feq = env.phase_density(phase_bins, vmin, vmax)[0]                 # the KL target: environment 0's initial density
    with env.recording(stride=stride, x_bins=100, v_bins=100, phase_bins=phase_bins, vmin=vmin, vmax=vmax, feq=feq,
                       capacity=steps // stride + 1) as session:
        env.record_now()                                               # t = 0
        env.step_feedback(steps)                                       # the closed loop, one call
    rec = session.record
    env.close()
    gamma = landau.damping_rate(rec, *t_linear)
    for e in range(num_envs):
        print(f"env {e}: growth rate over t in [{t_linear[0]}, {t_linear[1]}] = {gamma[e]:+.4f}   entropy {rec.entropy[0, e]:.5f} -> "
              f"{rec.entropy[-1, e]:.5f}   KL {rec.kl[0, e]:.3e} -> {rec.kl[-1, e]:.3e}")
    if out:
        rec.save(out)
        print(f"{len(rec)} records of {num_envs} environments -> {out}")
    return rec


if __name__ == "__main__":
    args = sys.argv[1:]
    kw = {k: int(v) for k, v in zip(("num_envs", "N", "steps", "stride"), args[:4])}
    if len(args) > 4:
        kw["out"] = args[4]
    run(**kw)
