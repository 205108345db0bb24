#!/usr/bin/env python3
"""G17: the reference's rollout analyses (src/interpret/landau.py, spectrum.py, the KL of src/control/objective.py and the field
energy of plot.py's plot_log_E) on the particle snapshots already stored in g13_simulate.npz.

Runs ONLY where the reference is available (make_golden.py's `_import_reference`, same numba shim); needs scikit-learn and
SciPy, which the reference imports.  Usage::

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_g17.py

Stores parameters and the reference's outputs only; the snapshots stay in g13_simulate.npz.  Prefixes: "fb_" = G13's
field-trajectory rollout (`snapshot`, CIC), "free_" = its free TSC rollout (`free_snapshot`; the reference's analyses
recompute a CIC field from it whatever the run's shape function was).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _import_reference, save  # noqa: E402

# (vmin, vmax, dv) of compute_numerical_entropy: its bin count is int(vmax - vmin / dv) as written.  "a": dv = 1, where that equals
# (vmax - vmin) / dv = 16; "b": int(10 + 25) = 35 bins, not the 50 (vmax - vmin) / dv would give.
ENTROPY_CHOICES = {"a": (-8.0, 8.0, 1.0), "b": (-10.0, 10.0, 0.4)}
KL_BINS, KL_VMIN, KL_VMAX = 32, -10.0, 10.0
BOUNCE_AMPLITUDES = np.array([0.01, 0.1, 0.5])
ANALYTIC = np.array([[0.3, 1.0, 1.0], [0.5, 1.0, 1.0], [0.4, 0.5, 0.25]])     # (k, v_th, n0)


def main():
    _import_reference()
    from src.control.objective import estimate_f, estimate_KL_divergence
    from src.env.util import compute_E, generate_grad, generate_laplacian
    from src.interpret.landau import (compute_bounce_time, compute_linear_damping_rate, compute_linear_damping_rate_analytic,
                                      compute_numerical_entropy)
    from src.interpret.spectrum import compute_E_k_spectrum

    g = np.load(os.path.join(OUT, "g13_simulate.npz"))
    L, n0 = float(g["L"]), float(g["n0"])
    out = dict(L=L, n0=n0, kl_bins=KL_BINS, kl_vmin=KL_VMIN, kl_vmax=KL_VMAX, bounce_amplitudes=BOUNCE_AMPLITUDES,
               analytic_inputs=ANALYTIC)
    for c, (vmin, vmax, dv) in ENTROPY_CHOICES.items():
        out[f"entropy_{c}_vmin"], out[f"entropy_{c}_vmax"], out[f"entropy_{c}_dv"] = vmin, vmax, dv
    for pre, snap_key, Ng, tmax in (("fb", "snapshot", int(g["Ng"]), float(g["tmax"])),
                                    ("free", "free_snapshot", int(g["free_Ng"]), float(g["free_tmax"]))):
        snap = g[snap_key]
        N, Nt = snap.shape[0] // 2, snap.shape[1]
        dx = L / Ng
        out[f"{pre}_Ng"], out[f"{pre}_dx"], out[f"{pre}_tmax"] = Ng, dx, tmax
        out[f"{pre}_damping_rate"] = compute_linear_damping_rate(tmax, n0, L, dx, Ng, snap)
        for c, (vmin, vmax, dv) in ENTROPY_CHOICES.items():
            out[f"{pre}_entropy_{c}"] = np.array([compute_numerical_entropy(n0, L, dx, Ng, vmin, vmax, dv, snap[:, t])
                                                  for t in range(Nt)])
        ks, Ek = compute_E_k_spectrum(n0, L, dx, Ng, snap, return_abs=False)
        out[f"{pre}_ks"], out[f"{pre}_Ek"] = ks, Ek
        feq = estimate_f(snap[:, :1], KL_BINS, L, KL_VMIN, KL_VMAX, n0)
        kdx, kdv = L / KL_BINS, (KL_VMAX - KL_VMIN) / KL_BINS
        out[f"{pre}_feq"] = feq
        out[f"{pre}_kl"] = np.array([estimate_KL_divergence(estimate_f(snap[:, t:t + 1], KL_BINS, L, KL_VMIN, KL_VMAX, n0), feq,
                                                            kdx, kdv) for t in range(Nt)])
        G, Lap = generate_grad(L, Ng), generate_laplacian(L, Ng)
        E_n0 = [compute_E(snap[:, t].reshape(-1, 1), dx, Ng, n0, L, N, G, Lap)[1] for t in range(Nt)]      # landau.py:67
        E_1 = [compute_E(snap[:, t].reshape(-1, 1), dx, Ng, 1.0, L, N, G, Lap)[1] for t in range(Nt)]      # plot.py:580
        out[f"{pre}_E2_t"] = np.array([np.sum(e.ravel() ** 2) * dx for e in E_n0])
        out[f"{pre}_mean_E2"] = np.array([np.mean(e.ravel() ** 2) for e in E_1])
    out["bounce_time"] = np.array([compute_bounce_time(a) for a in BOUNCE_AMPLITUDES])
    out["damping_rate_analytic"] = np.array([compute_linear_damping_rate_analytic(*row) for row in ANALYTIC])
    save("g17_interpret", **out)


if __name__ == "__main__":
    main()
