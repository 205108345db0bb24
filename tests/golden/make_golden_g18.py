#!/usr/bin/env python3
"""G18: the reference's other integrators (src/env/integration.py: symplectic_euler :50, verlet :54, forward_euler :8) in its own
PIC.update_state (pic.py:131-146), whose `symplectic_4th_order` is replaced by each of them in turn.

Runs ONLY where the reference is available (make_golden.py's `_import_reference`, same numba shim).  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_g18.py

Cases (prefix), each under every scheme (second prefix: se / vv / fe):
  ts   two-stream, N = 5000, Ng = 250, dt = 0.05, CIC, 200 steps
  bot  bump-on-tail, N = 1e4, Ng = 128, dt = 0.1, TSC, 100 steps
  ext  two-stream, N = 3000, Ng = 200, dt = 0.1, CIC, 50 steps under one constant E_field external field
  act  bump-on-tail, N = 4000, Ng = 256, dt = 0.1, CIC, 20 steps with a new action every step
Stored: parameters, the initial state after PIC.initialize, per step KE, PE, H (entry 0 = the initial state), E_mesh after
step 1, 10 and the last, and x, v of every MARK_STRIDE-th particle (indices 0, 8, 16, ...) after those steps -- the whole state
at three steps of four cases under three schemes would be 3.2 MB; the energy traces depend on every particle.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, save  # noqa: E402

SCHEMES = (("se", "symplectic_euler"), ("vv", "verlet"), ("fe", "forward_euler"))
MARK_STRIDE = 8
L = 50.0


def main():
    _import_reference()
    import src.env.integration as integ
    import src.env.pic as pic_module
    from src.control.actuator import E_field
    from src.env.dist import BumpOnTail, TwoStream
    from src.env.pic import PIC

    out = dict(L=L, mark_stride=MARK_STRIDE)

    def case(pre, make_dist, N, Ng, dt, K, interpol, seed, ext=None, actions=None):
        out.update({f"{pre}_N": N, f"{pre}_Ng": Ng, f"{pre}_dt_in": dt, f"{pre}_steps": K, f"{pre}_tsc": interpol == "TSC"})
        if ext is not None:
            out[f"{pre}_E_ext"] = ext
        if actions is not None:
            out[f"{pre}_actions"] = actions
        for tag, name in SCHEMES:
            pic_module.symplectic_4th_order = getattr(integ, name)      # update_state's integrator, nothing else
            np.random.seed(seed)
            sim = PIC(N=N, N_mesh=Ng, n0=1.0, L=L, dt=dt, tmin=0.0, tmax=50.0, gamma=5.0, A=0.1, n_mode=2,
                      interpol=interpol, init_dist=make_dist(N))
            if tag == "se":
                out.update({f"{pre}_dt": sim.dt, f"{pre}_x_init": sim.x.ravel().copy(), f"{pre}_v_init": sim.v.ravel().copy()})
            else:
                assert np.array_equal(out[f"{pre}_x_init"], sim.x.ravel())
            actu = E_field(L, Ng, 3)
            KE, PE, H = [0.5 * np.sum(sim.v * sim.v)], [sim.get_electric_energy()], [sim.get_energy()]
            for k in range(1, K + 1):
                E_ext = ext
                if actions is not None:
                    actu.update_E(actions[k - 1, :3], actions[k - 1, 3:])
                    E_ext = actu.compute_E()
                sim.update_state(E_ext)
                KE.append(0.5 * np.sum(sim.v * sim.v)); PE.append(sim.get_electric_energy()); H.append(sim.get_energy())
                if k in (1, 10, K):
                    out[f"{pre}_{tag}_x_{k}"] = sim.x.ravel()[::MARK_STRIDE].copy()
                    out[f"{pre}_{tag}_v_{k}"] = sim.v.ravel()[::MARK_STRIDE].copy()
                    out[f"{pre}_{tag}_E_mesh_{k}"] = sim.E_mesh.ravel().copy()
            out.update({f"{pre}_{tag}_KE": np.array(KE), f"{pre}_{tag}_PE": np.array(PE), f"{pre}_{tag}_H": np.array(H)})
        pic_module.symplectic_4th_order = integ.symplectic_4th_order

    case("ts", lambda N: TwoStream(v0=3.0, sigma=1.0, n_samples=N, L=L), 5000, 250, 0.05, 200, "CIC", 60)
    case("bot", lambda N: BumpOnTail(a=0.2, v0=3.0, sigma=1.0, n_samples=N, L=L), 10000, 128, 0.1, 100, "TSC", 61)
    rng = np.random.default_rng(62)
    act = E_field(L, 200, 3)
    act.update_E(rng.uniform(-1.25, 1.25, 3), rng.uniform(-1.25, 1.25, 3))
    case("ext", lambda N: TwoStream(v0=3.0, sigma=1.0, n_samples=N, L=L), 3000, 200, 0.1, 50, "CIC", 63,
         ext=np.asarray(act.compute_E()).reshape(-1, 1))
    case("act", lambda N: BumpOnTail(a=0.2, v0=3.0, sigma=1.0, n_samples=N, L=L), 4000, 256, 0.1, 20, "CIC", 64,
         actions=rng.uniform(-1.25, 1.25, (20, 6)))
    save("g18_integrators", **out)


if __name__ == "__main__":
    main()
