"""Rollout records (include/picstep.h: pic_record_*): what the reference's analyses take from a full ``(2N, Nt)`` particle
snapshot -- field energy, Fourier spectrum, x and v distributions, phase-space entropy and KL -- reduced on the device after
every ``stride``-th step of every environment and read back once.  ``BatchedPIC.start_recording`` / ``PIC.start_recording``
switch it on; ``interpret.landau`` works from the ``Record`` they return.
"""
from contextlib import contextmanager
from typing import Optional

import numpy as np


class Record:
    """Records of a rollout as NumPy arrays (R records, E environments, M spectrum rows):

    steps [R] (step index counted from start_recording), t = steps * dt [R];
    KE, PE, PE_reward, field_energy (= sum(E_mesh^2) dx), entropy, kl, inside [R, E];
    Ek complex [R, E, M] (rows 0..M-1 of fft(E_mesh) / N_mesh * 2) and ks [M] (their wavenumbers, 2 pi fftfreq);
    x_hist [R, E, x_bins] on [0, L], v_hist [R, E, v_bins] on [vmin, vmax] (uint32 counts), x_edges / v_edges.
    entropy and kl are NaN where no phase histogram (or, for kl, no target density) was configured."""

    _ARRAYS = ("steps", "t", "KE", "PE", "PE_reward", "field_energy", "entropy", "kl", "inside", "Ek", "ks", "x_hist", "v_hist",
               "x_edges", "v_edges")

    def __init__(self, **arrays):
        for k in self._ARRAYS:
            setattr(self, k, arrays[k])
        self.dt = float(arrays["dt"])

    @classmethod
    def _from_read(cls, raw, dt, L, N_mesh, vmin, vmax):
        n_modes = raw["re"].shape[2]
        xb, vb = raw["x_hist"].shape[2], raw["v_hist"].shape[2]
        dx = L / N_mesh
        ks = np.arange(n_modes) * (1.0 / (N_mesh * dx)) * 2.0 * np.pi       # np.fft.fftfreq(N_mesh, d=dx) * 2 pi, rows 0..M-1
        return cls(steps=raw["step"], t=raw["step"] * dt, KE=raw["KE"], PE=raw["PE"], PE_reward=raw["PE_reward"],
                   field_energy=raw["field_energy"], entropy=raw["entropy"], kl=raw["kl"], inside=raw["inside"],
                   Ek=raw["re"] + 1j * raw["im"], ks=ks, x_hist=raw["x_hist"], v_hist=raw["v_hist"],
                   x_edges=np.linspace(0, L, xb + 1) if xb else np.empty(0),
                   v_edges=np.linspace(vmin, vmax, vb + 1) if vb else np.empty(0), dt=dt)

    def __len__(self):
        return len(self.steps)

    def save(self, path):
        """-> .npz with every array and dt."""
        np.savez(path, dt=self.dt, **{k: getattr(self, k) for k in self._ARRAYS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(**{k: z[k] for k in z.files})


class RecordingSession:
    """What ``recording(...)`` yields: ``record`` holds the Record once the block has ended."""
    record: Optional[Record] = None


def recorder_args(N_mesh, stride, modes, x_bins, v_bins, phase_bins, vmin, vmax, feq, capacity, phase_dx=0.0, phase_dv=0.0):
    """The Python spellings -> Handle.record_start keywords.  modes None = the non-negative wavenumbers of
    compute_E_k_spectrum ((N_mesh + 1) // 2 rows); phase_bins None = none, an int = square, or (x_bins, v_bins)."""
    if phase_bins is None:
        pb = (0, 0)
    elif np.ndim(phase_bins) == 0:
        pb = (int(phase_bins), int(phase_bins))
    else:
        pb = tuple(int(b) for b in phase_bins)
    return dict(stride=stride, n_modes=(int(N_mesh) + 1) // 2 if modes is None else int(modes), x_bins=x_bins, v_bins=v_bins,
                phase_bins=pb, vmin=vmin, vmax=vmax, phase_dx=phase_dx, phase_dv=phase_dv, feq=feq, capacity=capacity)


@contextmanager
def recording_session(env, **kwargs):
    env.start_recording(**kwargs)
    session = RecordingSession()
    try:
        yield session
    finally:
        try:
            session.record = env.recorded()
        finally:
            env.stop_recording()
