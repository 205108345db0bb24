"""Host-side checks of the other integrators (include/picstep.h: pic_set_integrator) and of the G18 fixture (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import hp_integrators as hpi
from hp_reference import LD, energies, solve, deposit
from ocplasma_amd import _abi, _build

TAGS = {"se": "symplectic_euler", "vv": "verlet", "fe": "forward_euler"}


@pytest.fixture(scope="module")
def lib_path():
    return _build.build_library()


@pytest.fixture(scope="module")
def g18():
    return load_golden("g18_integrators")


def _header():
    return open(os.path.join(ROOT, "include", "picstep.h")).read()


def test_header_enum_and_entries(lib_path):
    hdr = _header()
    body = hdr[hdr.index("enum { PIC_YOSHIDA4"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("};")], flags=re.S)
    pairs = dict((k, int(v)) for k, v in re.findall(r"(PIC_\w+)\s*=\s*(\d+)", body))
    assert pairs == {"PIC_YOSHIDA4": _abi.PIC_YOSHIDA4, "PIC_SYMPLECTIC_EULER": _abi.PIC_SYMPLECTIC_EULER,
                     "PIC_VERLET": _abi.PIC_VERLET, "PIC_FORWARD_EULER": _abi.PIC_FORWARD_EULER}
    declared = set(re.findall(r"^int\s+(pic_\w+_integrator)\s*\(", hdr, re.M))
    assert declared == {"pic_set_integrator", "pic_get_integrator"}
    lib = ctypes.CDLL(lib_path)
    for name in declared:
        assert hasattr(lib, name), name


def test_ctypes_signatures():
    assert _abi.SIGNATURES["pic_set_integrator"] == [ctypes.c_void_p, ctypes.c_int]
    assert _abi.SIGNATURES["pic_get_integrator"] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    hdr = _header()
    assert re.search(r"int pic_set_integrator\(pic_handle\* h, int scheme\);", hdr)
    assert re.search(r"int pic_get_integrator\(pic_handle\* h, int\* scheme, int\* evals_per_step\);", hdr)


def test_abi_version_still_5(lib_path):
    assert "#define PICSTEP_ABI_VERSION 5" in _header()
    assert _abi.ABI_VERSION == 5 and ctypes.CDLL(lib_path).pic_abi_version() == 5


def test_default_is_yoshida4():
    import inspect
    from ocplasma_amd.env.batched import BatchedPIC
    from ocplasma_amd.env.pic import PIC
    for fn in (PIC.__init__, BatchedPIC.__init__, _abi.Handle.__init__):
        assert inspect.signature(fn).parameters["integrator"].default == "symplectic_4th_order"
    assert _abi.integrator_id("symplectic_4th_order") == _abi.PIC_YOSHIDA4 == 0


def test_name_and_function_mapping():
    for name, scheme in (("symplectic_4th_order", 0), ("symplectic_euler", 1), ("verlet", 2), ("forward_euler", 3)):
        assert _abi.integrator_id(name) == scheme
        fn = lambda eta, grad, dt: eta   # noqa: E731  (a stand-in with the reference's name)
        fn.__name__ = name
        assert _abi.integrator_id(fn) == scheme
        assert _abi.INTEGRATOR_NAMES[scheme] == name
    assert [_abi.EVALS_PER_STEP[s] for s in range(4)] == [3, 1, 2, 1]


@pytest.mark.parametrize("bad", ["implicit_midpoint", "explicit_midpoint", "Verlet", "", None, 2, print])
def test_unknown_integrator_raises(bad):
    with pytest.raises(ValueError):
        _abi.integrator_id(bad)


def test_pic_rejects_unknown_integrator_before_touching_the_device():
    from ocplasma_amd.env.pic import PIC
    with pytest.raises(ValueError):
        PIC(N=100, N_mesh=16, integrator="implicit_midpoint")


# ---- hp_integrators against G18 (the reference's own float64 runs) ------------------------------------------------------
# A float64 step differs from the longdouble one by a few ulps of the positions and velocities; over k steps the difference
# grows with the system's sensitivity.  Bounds are 100 x the worst measured over all cases and schemes: x / L and v relative to
# max|v| after step 1: 7.7e-16, after step 10: 6.1e-15; E_mesh relative to max|E_mesh|: 8.2e-14 (the reference's
# Sherman-Morrison solve against cumulative sums); over the first ten steps KE 1.9e-15 and PE 2.1e-13 relative.
@pytest.mark.parametrize("case", ["ts", "bot", "ext", "act"])
@pytest.mark.parametrize("tag", sorted(TAGS))
def test_hp_integrators_against_g18(g18, case, tag):
    L = float(g18["L"])
    N, Ng, dt = int(g18[f"{case}_N"]), int(g18[f"{case}_Ng"]), float(g18[f"{case}_dt"])
    shape = "TSC" if bool(g18[f"{case}_tsc"]) else "CIC"
    x, v = g18[f"{case}_x_init"], g18[f"{case}_v_init"]
    ext = g18[f"{case}_E_ext"].ravel() if f"{case}_E_ext" in g18.files else None
    ext_list = None
    if f"{case}_actions" in g18.files:
        from ocplasma_amd.control.actuator import E_field
        act = E_field(L, Ng, 3)
        ext_list = []
        for a in g18[f"{case}_actions"][:10]:
            act.update_E(a[:3], a[3:])
            ext_list.append(np.asarray(act.compute_E()).ravel())
    KE, PE = [], []
    for k in range(1, 11):
        e = ext_list[k - 1] if ext_list is not None else ext
        x, v, _ = hpi.scheme_step(TAGS[tag], x, v, e, dt, Ng, L, 1.0, N, shape)
        n, _ = deposit(x, Ng, L, 1.0, N, shape)
        E, _ = solve(n, 1.0, L)
        ke, pe, _ = energies(v, E, L, N)
        KE.append(ke)
        PE.append(pe)
        if k in (1, 10):
            bound = 7.7e-14 if k == 1 else 6.1e-13
            xr, vr = g18[f"{case}_{tag}_x_{k}"], g18[f"{case}_{tag}_v_{k}"]     # every mark_stride-th particle
            ms = int(g18["mark_stride"])
            dxs = np.abs(x[::ms].astype(float) - xr)
            dxs = np.minimum(dxs, L - dxs)
            assert dxs.max() / L < bound, (k, dxs.max())
            assert np.abs(v[::ms].astype(float) - vr).max() / np.abs(vr).max() < bound
            Er = g18[f"{case}_{tag}_E_mesh_{k}"]
            assert np.abs(E.astype(float) - Er).max() / np.abs(Er).max() < 8.2e-12
    assert np.allclose(np.array(KE, dtype=float), g18[f"{case}_{tag}_KE"][1:11], rtol=1.9e-13, atol=0)
    assert np.allclose(np.array(PE, dtype=float), g18[f"{case}_{tag}_PE"][1:11], rtol=2.1e-11, atol=0)


def test_g18_schemes_differ_and_verlet_conserves_best(g18):
    """Sanity of the fixture itself: the three schemes make different trajectories, and over the two-stream run Verlet's
    energy drift is the smallest of the three, forward Euler's the largest (it is not symplectic)."""
    drift = {tag: np.abs(g18[f"ts_{tag}_H"] - g18[f"ts_{tag}_H"][0]).max() for tag in TAGS}
    assert drift["vv"] < drift["se"] < drift["fe"]
    assert not np.array_equal(g18["ts_se_x_1"], g18["ts_vv_x_1"])
