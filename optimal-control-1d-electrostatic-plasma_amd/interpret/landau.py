"""Landau damping / growth diagnostics with the reference's names and signatures (``src/interpret/landau.py``), plus the same
analyses computed from a rollout ``Record`` (``BatchedPIC.start_recording``) instead of a ``(2N, Nt)`` particle snapshot.

The snapshot functions evaluate on the device through a single-environment probe handle: each column is loaded and reduced by
``pic_record_now`` (deposit -> field solve -> sum(E_mesh^2) dx, or the phase-space histogram and its entropy).  The fit is an
ordinary least-squares line in NumPy (the reference uses scikit-learn's LinearRegression, which computes the same line).

What the numbers mean.  The reference recomputes a CIC field from the positions with the ``n0`` it is given (``plot_log_E``
passes ``n0 = 1``, ``compute_linear_damping_rate`` the caller's).  A Record holds the environment's own ``E_mesh``: the two agree
for CIC environments with the same ``n0`` -- for ``plot_log_E`` that means ``n0 = 1``, which is what the reference's runs use.
"""
import numpy as np

from ..control.reward import _probe


def compute_bounce_time(perturbed_amplitude: float):
    """landau.py:5-14 as written: 1 / sqrt(amplitude) (its docstring's 2 pi factor is not in the code)."""
    return 1.0 / np.sqrt(perturbed_amplitude)


def compute_linear_damping_rate_analytic(k: float, v_th: float, n0: float):
    """Linear Landau damping rate of a Langmuir wave, valid for k lambda_De << 1 (landau.py:28-43)."""
    w_pe = np.sqrt(4 * np.pi * n0)
    lamda_de = v_th / w_pe
    kl = k * lamda_de
    return np.exp(-1 / (2 * kl ** 2)) / kl ** 3 * np.sqrt(np.pi / 8) * w_pe


def _columns(snapshot):
    snap = np.asarray(snapshot, dtype=np.float64)
    if snap.ndim == 1:
        snap = snap.reshape(-1, 1)
    return snap, snap.shape[0] // 2


def compute_numerical_entropy(n0: float, L: float, dx: float, N_mesh: float, vmin: float, vmax: float, dv: float,
                              snapshot: np.ndarray, device: int = 0):
    """-sum_{f>0} f ln f dx dv of the phase-space density of ONE state [x; v] (landau.py:16-26): an np.histogram2d of
    [N_mesh, int(vmax - vmin / dv)] bins on [0, L] x [vmin, vmax] -- that bin count as the reference writes it, operator
    precedence included -- normalised by the GIVEN dx and dv, f = counts n0 / dx / dv / N."""
    snap, n = _columns(snapshot)
    nv = int(vmax - vmin / dv)
    h = _probe(n, int(N_mesh), L, n0, device)
    h.reset(snap[:n, 0].reshape(1, n), snap[n:2 * n, 0].reshape(1, n))
    h.record_start(n_modes=0, phase_bins=(int(N_mesh), nv), vmin=vmin, vmax=vmax, phase_dx=dx, phase_dv=dv, capacity=1)
    try:
        h.record_now()
        return float(h.record_read()["entropy"][0, 0])
    finally:
        h.record_stop()


def _field_energy_columns(n0, L, N_mesh, snapshot, device):
    """sum(E_mesh^2) dx of the CIC field of every column (landau.py:67-68), one pic_record_now each."""
    snap, n = _columns(snapshot)
    h = _probe(n, int(N_mesh), L, n0, device)
    h.record_start(n_modes=0, capacity=snap.shape[1])
    try:
        for t in range(snap.shape[1]):
            h.reset(snap[:n, t].reshape(1, n), snap[n:2 * n, t].reshape(1, n))
            h.record_now()
        return h.record_read()["field_energy"][:, 0]
    finally:
        h.record_stop()


def _ols_slope(t, y):
    t = np.asarray(t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    tc = t - t.mean()
    return float(np.dot(tc, y - y.mean()) / np.dot(tc, tc))


def compute_linear_damping_rate(tmax: float, n0: float, L: float, dx: float, N_mesh: float, snapshot: np.ndarray,
                                device: int = 0):
    """0.5 x the slope of log(sum(E_mesh^2) dx) against ts = linspace(0, tmax, Nt) over the Nt columns of a (2N, Nt) snapshot
    (landau.py:45-80; log E^2 = 2 gamma t + C)."""
    snap, _ = _columns(snapshot)
    ts = np.linspace(0, tmax, snap.shape[1])
    return 0.5 * _ols_slope(ts, np.log(_field_energy_columns(n0, L, N_mesh, snap, device)))


# -- the same analyses from a Record --------------------------------------------------------------------------------------------
def damping_rate(record, t_from=None, t_to=None):
    """Per environment, 0.5 x the least-squares slope of log(field_energy) against the record's true times t = steps * dt,
    restricted to t_from <= t <= t_to (e.g. the linear phase) -> [E].  compute_linear_damping_rate differs only in its time
    axis: it spreads its Nt columns evenly over [0, tmax] whatever steps they were taken at."""
    t = np.asarray(record.t, dtype=np.float64)
    keep = np.ones(t.shape, dtype=bool)
    if t_from is not None:
        keep &= t >= t_from
    if t_to is not None:
        keep &= t <= t_to
    if keep.sum() < 2:
        raise ValueError("damping_rate: fewer than two records in the time window")
    logE2 = np.log(np.asarray(record.field_energy)[keep])
    return np.array([0.5 * _ols_slope(t[keep], logE2[:, e]) for e in range(logE2.shape[1])])


def E_k_spectrum(record):
    """compute_E_k_spectrum's result from a Record: (ks [M], |E_k| [E, M, R]) -- per environment one row per wavenumber and
    one column per record, as the reference lays out its (k, t) matrix."""
    return record.ks, np.abs(np.asarray(record.Ek)).transpose(1, 2, 0)
