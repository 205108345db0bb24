"""Host-side checks of the rollout recorder (include/picstep.h: pic_record_*) and of the G17 fixture (no GPU needed)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden

from ocplasma_amd import _abi, _build
from ocplasma_amd.interpret import landau

RECORD_STRUCTS = (("pic_record_config", _abi.PicRecordConfig), ("pic_record_out", _abi.PicRecordOut))


@pytest.fixture(scope="module")
def lib_path():
    return _build.build_library()


def _header():
    return open(os.path.join(ROOT, "include", "picstep.h")).read()


@pytest.mark.parametrize("name,cls", RECORD_STRUCTS)
def test_record_struct_fields_match_header(name, cls):
    hdr = _header()
    body = hdr[hdr.index(f"typedef struct {name} {{") + len(f"typedef struct {name} {{"):hdr.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"const", "int32_t", "int64_t", "uint32_t", "double", ","}
    fields = [t for stmt in body.split(";")[:-1] for t in stmt.replace("*", " ").replace(",", " , ").split() if t not in types]
    assert fields == [f[0] for f in cls._fields_], fields


def test_record_struct_offsets_match_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = []
    for name, cls in RECORD_STRUCTS:
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'  printf("{name} {f} %zu\\n", offsetof({name}, {f}));')
    src = tmp_path / "offsets.c"
    src.write_text('#include "picstep.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + "\n".join(lines) +
                   "\n  return 0;\n}\n")
    exe = tmp_path / "offsets"
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for name, cls in RECORD_STRUCTS:
        want.append(f"{name} sizeof {ctypes.sizeof(cls)}")
        want += [f"{name} {f} {getattr(cls, f).offset}" for f, _ in cls._fields_]
    assert got[:-1] == want


def test_record_entries_declared_and_exported(lib_path):
    hdr = _header()
    declared = set(re.findall(r"^int\s+(pic_record_\w+)\s*\(", hdr, re.M))
    assert declared == {"pic_record_start", "pic_record_now", "pic_record_count", "pic_record_read", "pic_record_stop"}
    assert declared <= set(_abi.SIGNATURES)
    lib = ctypes.CDLL(lib_path)
    for name in declared:
        assert hasattr(lib, name), name
    assert "#define PICSTEP_ABI_VERSION 5" in hdr
    assert _abi.ABI_VERSION == 5 and lib.pic_abi_version() == _abi.ABI_VERSION


def test_header_with_recorder_is_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_recorder.c"
    src.write_text('#include "picstep.h"\n#include <stddef.h>\n'
                   "int main(void) {\n  pic_record_config c = {0};\n  pic_record_out o = {0};\n  int64_t n = 0;\n"
                   "  c.stride = 10; c.n_modes = 8; c.x_bins = 64; c.v_bins = 64; c.phase_x_bins = 64; c.phase_v_bins = 32;\n"
                   "  c.vmin = -25.0; c.vmax = 25.0; c.feq = NULL; c.capacity = 100;\n"
                   "  void* fns[] = {(void*)&pic_record_start, (void*)&pic_record_now, (void*)&pic_record_count,\n"
                   "                  (void*)&pic_record_read, (void*)&pic_record_stop};\n"
                   "  (void)fns; (void)o; (void)n;\n  return c.stride - 10;\n}\n")
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-Wno-pedantic", "-I", os.path.join(ROOT, "include"),
                        "-c", str(src), "-o",
                        str(tmp_path / "use_recorder.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_landau_host_formulas_equal_g17():
    g = load_golden("g17_interpret")
    got = np.array([landau.compute_bounce_time(a) for a in g["bounce_amplitudes"]])
    assert np.array_equal(got, g["bounce_time"])
    got = np.array([landau.compute_linear_damping_rate_analytic(*row) for row in g["analytic_inputs"]])
    np.testing.assert_allclose(got, g["damping_rate_analytic"], rtol=1e-14, atol=0)


def _entropy_np(n0, L, dx, Ng, vmin, vmax, dv, state):
    n = state.shape[0] // 2
    nv = int(vmax - vmin / dv)               # landau.py's bin count as written
    h = np.histogram2d(state[:n], state[n:], bins=[Ng, nv], range=[[0, L], [vmin, vmax]])[0]
    f = h * (n0 / dx / dv / n)
    f = f[f != 0]
    return -(f * np.log(f)).sum() * dx * dv


@pytest.mark.parametrize("pre,snap_key", [("fb", "snapshot"), ("free", "free_snapshot")])
def test_g17_entropies_follow_from_g13_snapshots(pre, snap_key):
    """np.histogram2d of the snapshots G13 stores reproduces G17's entropies, at both (vmin, vmax, dv) choices -- including
    the one where int(vmax - vmin / dv) is not (vmax - vmin) / dv."""
    g13, g = load_golden("g13_simulate"), load_golden("g17_interpret")
    snap = g13[snap_key]
    L, n0, Ng, dx = float(g["L"]), float(g["n0"]), int(g[f"{pre}_Ng"]), float(g[f"{pre}_dx"])
    for c in ("a", "b"):
        vmin, vmax, dv = (float(g[f"entropy_{c}_{k}"]) for k in ("vmin", "vmax", "dv"))
        got = np.array([_entropy_np(n0, L, dx, Ng, vmin, vmax, dv, snap[:, t]) for t in range(snap.shape[1])])
        np.testing.assert_allclose(got, g[f"{pre}_entropy_{c}"], rtol=1e-13, atol=0)
    assert int(float(g["entropy_b_vmax"]) - float(g["entropy_b_vmin"]) / float(g["entropy_b_dv"])) == 35


def test_damping_rate_of_a_record_is_the_ols_slope():
    """interpret.landau.damping_rate on a hand-made record: 0.5 x slope of log(field_energy) against steps * dt, per
    environment, over the requested window."""
    from ocplasma_amd.interpret import Record
    steps = np.arange(0, 40, 2)
    dt = 0.1
    gam = np.array([0.3, -0.2])
    fe = np.exp(2 * gam[None, :] * (steps * dt)[:, None] + np.array([0.5, -1.0]))
    z = np.zeros((len(steps), 2))
    rec = Record(steps=steps, t=steps * dt, KE=z, PE=z, PE_reward=z, field_energy=fe, entropy=z, kl=z, inside=z.astype(np.int64),
                 Ek=np.zeros((len(steps), 2, 3), complex), ks=np.arange(3.0), x_hist=np.zeros((len(steps), 2, 0), np.uint32),
                 v_hist=np.zeros((len(steps), 2, 0), np.uint32), x_edges=np.empty(0), v_edges=np.empty(0), dt=dt)
    np.testing.assert_allclose(landau.damping_rate(rec), gam, rtol=1e-12)
    np.testing.assert_allclose(landau.damping_rate(rec, t_from=1.0, t_to=2.0), gam, rtol=1e-12)
    ks, ek = landau.E_k_spectrum(rec)
    assert ek.shape == (2, 3, len(steps))
