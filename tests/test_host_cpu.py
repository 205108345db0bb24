"""CPU-only checks of the host layer: samplers vs the reference's RNG stream, actuator, the C-ABI
library's exports, and that the product path refuses to run without a GPU (no fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden, rel_err

import ocplasma_amd
from ocplasma_amd import _abi, _build
from ocplasma_amd.control.actuator import E_field
from ocplasma_amd.control.reward import Reward, estimate_f, estimate_KL_divergence
from ocplasma_amd.env.dist import BumpOnTail, TwoStream


@pytest.fixture(scope="module")
def lib_path():
    return _build.build_library()


def test_samplers_reproduce_reference_stream():
    g = load_golden("g10_samplers")
    n, L = int(g["n"]), float(g["L"])
    np.random.seed(int(g["seed"]))
    ts = TwoStream(v0=3.0, sigma=1.0, n_samples=n, L=L)
    x1, v1 = ts.get_sample()
    ts.reinit()
    x2, v2 = ts.get_sample()
    assert np.array_equal(x1, g["ts_x1"]) and np.array_equal(v1, g["ts_v1"])
    assert np.array_equal(x2, g["ts_x2"]) and np.array_equal(v2, g["ts_v2"])
    assert np.array_equal(ts.get_init_state(), g["ts_init_state"])
    np.random.seed(int(g["seed"]))
    bt = BumpOnTail(a=0.2, v0=3.0, sigma=1.0, n_samples=n, L=L)
    x1, v1 = bt.get_sample()
    bt.reinit()
    x2, v2 = bt.get_sample()
    assert np.array_equal(x1, g["bt_x1"]) and np.array_equal(v1, g["bt_v1"])
    assert np.array_equal(x2, g["bt_x2"]) and np.array_equal(v2, g["bt_v2"])
    assert np.array_equal(bt.high_indx, g["bt_high_indx"])
    assert np.array_equal(bt.get_init_state(), g["bt_init_state"])


def test_sampler_trajectory_inputs_match_golden():
    """The x0/v0 the reference drew for the g5 trajectory (seed 42, then PIC.__init__'s redraw)."""
    g = load_golden("g5_bump_on_tail_N10000_Ng128")
    np.random.seed(42)
    d = BumpOnTail(a=0.2, v0=3.0, sigma=1.0, n_samples=10000, L=50.0)
    d.reinit()     # PIC.initialize redraws (pic.py:64)
    assert np.array_equal(d.x_init, g["x0_raw"]) and np.array_equal(d.v_init, g["v0_raw"])


def test_actuator_matches_golden():
    g = load_golden("g8_actuator")
    for Ng, mm in ((128, 3), (250, 5), (256, 1)):
        a = E_field(float(g["L"]), Ng, mm)
        E = a.compute_E(g[f"cc_{Ng}_{mm}"], g[f"cs_{Ng}_{mm}"])
        assert E.shape == (Ng, 1) and np.array_equal(E, g[f"E_{Ng}_{mm}"])
        a.update_E(g[f"cc_{Ng}_{mm}"], g[f"cs_{Ng}_{mm}"])
        assert np.array_equal(a.compute_E(), E)
        acts = np.concatenate([g[f"cc_{Ng}_{mm}"], g[f"cs_{Ng}_{mm}"]])[None]
        assert rel_err(a.compute_E_batched(acts)[0], E) < 1e-14
        a.reinit()
        assert not a.coeff_cos.any()


def test_reward_host_pieces():
    rng = np.random.default_rng(0)
    st = np.concatenate([rng.uniform(0, 50, 500), rng.normal(0, 1, 500)]).reshape(-1, 1)
    f = estimate_f(st, 32, 50.0, -25.0, 25.0, 1.0)
    assert f.shape == (32, 32) and abs(f.sum() * (50 / 32) * (50 / 32) - 1.0) < 1e-9
    assert abs(estimate_KL_divergence(f, f.copy(), 50 / 32, 50 / 32)) < 1e-6
    r = Reward.__new__(Reward)
    r.L = 50.0
    assert r.compute_input_energy(np.ones(10)) == 10 * 50.0 * 0.25


def test_kl_diagnostic_matches_golden():
    g = load_golden("g11_phase_hist")
    nb, L = int(g["nbins"]), float(g["L"])
    rw = Reward.__new__(Reward)        # host-only pieces: no device handle needed
    rw.init_state, rw.N_mesh, rw.L, rw.vmin, rw.vmax, rw.n0 = g["st0"], nb, L, float(g["vmin"]), float(g["vmax"]), 1.0
    rw.reinit()
    for k in ("0", "1", "2"):
        f = estimate_f(g["st" + k], nb, L, -25.0, 25.0, 1.0)
        assert np.array_equal(f, g["f" + k]), k
        assert abs(rw.compute_kl_divergence(g["st" + k]) - float(g["kl" + k])) <= 1e-12 * max(1.0, abs(float(g["kl" + k])))


def test_header_symbols_are_exported(lib_path):
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(pic_[A-Za-z_]+)\s*\(", hdr, re.M))
    assert declared == set(_abi.SIGNATURES), declared ^ set(_abi.SIGNATURES)
    lib = ctypes.CDLL(lib_path)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pic_abi_version() == _abi.ABI_VERSION
    # ... and nothing else of the library's own: every helper has internal linkage.  What the toolchain adds stays: the HIP
    # compilation-unit id (__hip_cuid_<hash>) and the weak out-of-line copies of libstdc++ templates the host code instantiates
    # (std::vector<int>::push_back and ::_M_fill_assign, std::vector<char>::_M_fill_assign, std::to_string(int / long / unsigned long),
    # std::string(const char*, const allocator&), four operator+ on std::string), all mangled _ZNSt... or _ZSt...
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    toolchain = {s for s in exported if s.startswith(("__hip_cuid_", "_ZNSt", "_ZSt"))}
    assert exported - toolchain == declared, (exported - toolchain) ^ declared


def test_no_kernel_spills_registers(lib_path):
    """A particle loop that spills runs at a fraction of its speed and computes the same bits: no parity test notices (round 3
    shipped a float32 x 16-per-lane resident kernel with 1.5 KB of scratch per lane for a while: 114 us per step instead of 16).
    The build writes the compiler's resource report next to the library; every kernel in it must be scratch-free and the sweeps
    must keep the registers for eight waves per SIMD."""
    import json
    from ocplasma_amd import _build
    assert os.path.getmtime(_build.RESOURCES) >= os.path.getmtime(lib_path) - 120, "resource report older than the library"
    rep = json.load(open(_build.RESOURCES))
    assert len(rep) > 100
    # a report that could not be parsed (a compiler update rewording its remarks) must fail here, not pass as "no scratch"
    unparsed = {k: v for k, v in rep.items()
                if any(v.get(f) is None for f in ("scratch_bytes_per_lane", "vgprs", "waves_per_simd", "lds_bytes_per_block"))}
    assert not unparsed, unparsed
    spilled = {k: v["scratch_bytes_per_lane"] for k, v in rep.items() if v["scratch_bytes_per_lane"] != 0}
    assert not spilled, spilled
    for k, v in rep.items():
        if "sweep_kernel" in k:
            assert v["vgprs"] <= 64, (k, v)              # 512 VGPRs per SIMD lane / 8 waves
        m = re.search(r"resident_kernel.*Li(\d+)ELi8ELb([01])E", k)
        if m:     # the kernel without carried cells shares a CU with a second workgroup up to 10 particles per lane (picstep.hip: res_lean)
            assert v["vgprs"] <= (128 if m.group(2) == "0" and int(m.group(1)) <= 10 else 256), (k, v)


def test_placement_struct_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    body = hdr[hdr.index("typedef struct {\n  int32_t pairs_timed;"):hdr.index("} pic_placement;")]
    fields = [f for decl in re.findall(r"^\s*(?:int32_t|double)\s+([\w, ]+);", body, re.M) for f in decl.replace(" ", "").split(",")]
    assert fields == [f[0] for f in _abi._Placement._fields_], fields
    assert ctypes.sizeof(_abi._Placement) == 4 * 4 + 6 * 8


def test_sharded_env_resolves_its_device_once(monkeypatch):
    """ShardedPIC without `device`: the ordinal checked across ranks must be the ordinal the handle is created on (a rank that
    only called torch.cuda.set_device(LOCAL_RANK) used to pass the check with its current device and build on device 0)."""
    import torch
    import torch.distributed as dist
    from ocplasma_amd.env import sharded
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_backend", lambda *a: "nccl")
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(dist, "get_rank", lambda *a: 1)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 5)
    seen = {}

    def all_gather_object(out, mine):
        seen["mine"] = mine
        out[0], out[1] = ("host", 4), mine

    monkeypatch.setattr(dist, "all_gather_object", all_gather_object)

    def factory(num_envs, N, Ng, **kw):
        seen["kw"] = kw
        return object()

    sh = sharded.ShardedPIC(6, 100, 16, env_factory=factory)
    assert seen["mine"][1] == 5 and seen["kw"]["device"] == 5 and sh.device == 5
    sh = sharded.ShardedPIC(6, 100, 16, env_factory=factory, device=3)
    assert seen["mine"][1] == 3 and seen["kw"]["device"] == 3
    # two ranks that resolve to the same device of the same host are refused

    def clash(out, mine):
        out[0], out[1] = mine, mine

    monkeypatch.setattr(dist, "all_gather_object", clash)
    with pytest.raises(RuntimeError, match="both drive device"):
        sharded.ShardedPIC(6, 100, 16, env_factory=factory)


def test_config_struct_layout_matches_header():
    # int64 N; int32 Ng, num_envs; 4 doubles; 9 int32 (+ 4 bytes of tail padding to the 8-byte alignment)
    assert ctypes.sizeof(_abi.PicConfig) == 8 + 4 + 4 + 4 * 8 + 9 * 4 + 4
    hdr = open(os.path.join(ROOT, "include", "picstep.h")).read()
    body = hdr[hdr.index("typedef struct pic_config {"):hdr.index("} pic_config;")]
    fields = re.findall(r"^\s*(?:int64_t|int32_t|double)\s+(\w+);", body, re.M)
    assert fields == [f[0] for f in _abi.PicConfig._fields_], fields


def test_no_cpu_fallback(lib_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_abi.PicError, match="no HIP device"):
        _abi.Handle(1000, 64)
    from ocplasma_amd.env.pic import PIC

    class D:
        def reinit(self): pass
        def get_sample(self): return np.zeros(100), np.zeros(100)
    with pytest.raises(_abi.PicError):
        PIC(N=100, N_mesh=16, dt=0.1, init_dist=D())


def test_bad_config_is_rejected(lib_path):
    lib = _abi.load()
    cfg = _abi.PicConfig(0, 64, 1, 50.0, 1.0, 0.1, 5.0, 0, 0, 0, 0, 0, 0, 0, 0)
    h = ctypes.c_void_p()
    assert lib.pic_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"N>=1" in lib.pic_last_error(None)
    A = _abi
    cfg = A.PicConfig(100, 64, 1, 50.0, 1.0, 0.1, 5.0, A.PIC_F64, 7, 0, 0, 0, 0, 0, 0)                  # no such accumulator
    assert lib.pic_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    cfg = A.PicConfig(100, 64, 1, 50.0, 1.0, 0.1, 5.0, A.PIC_F64, A.PIC_ACC_PACKED, 0, 0, 0, 0, 0, 0)   # packed word, f64 particles
    assert lib.pic_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"float32 particles" in lib.pic_last_error(None)
    cfg = A.PicConfig(100, 64, 1, 50.0, 1.0, 0.1, 5.0, A.PIC_F32, A.PIC_ACC_PACKED, A.PIC_TSC, 0, 0, 0, 0, 0)   # packed word, TSC
    assert lib.pic_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"CIC only" in lib.pic_last_error(None)
    cfg = A.PicConfig(100, 64, 1, 50.0, 1.0, 0.1, 5.0, A.PIC_F32, A.PIC_ACC_F64, 0, 0, 0, 0, 0, 0)      # f64 LDS sums, f32 particles
    assert lib.pic_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"float64 particles" in lib.pic_last_error(None)
    cfg = A.PicConfig(100, 64, 1, 50.0, 1.0, 0.1, 5.0, A.PIC_F64, 0, 0, 0, 0, 0, A.PIC_POS_FIXED32, 0)  # fixed-point x, f64 particles
    assert lib.pic_create(ctypes.byref(cfg), ctypes.byref(h)) == -1
    assert b"fixed-point positions" in lib.pic_last_error(None)
    with pytest.raises(ValueError, match="accum_dtype"):
        A.Handle(100, 64, accum_dtype="float32")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "optimal-control-1d-electrostatic-plasma_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                assert "oracle" not in open(os.path.join(dp, f)).read(), f


def test_dense_operator_mirrors_and_solver_argument_checks():
    """env/util.generate_grad / generate_laplacian are bit-identical to the oracle's (which the golden vectors pin
    through the reference's solves); solve.Gaussian_Elimination_Periodic rejects what the device solver does not
    handle before anything touches the GPU."""
    from ocplasma_amd.env import solve, util
    from oracle import pic_oracle as po
    for L, Ng in ((50.0, 8), (50.0, 250), (10.0, 129)):
        assert np.array_equal(util.generate_grad(L, Ng), po.dense_grad(L, Ng))
        assert np.array_equal(util.generate_laplacian(L, Ng), po.dense_laplacian(L, Ng))
        assert abs(solve._laplacian_spacing(util.generate_laplacian(L, Ng)) / (L / Ng) - 1) < 1e-15
    for bad in (np.eye(16), np.zeros((16, 16)), np.ones((4, 5)), util.generate_grad(50.0, 16),
                util.generate_laplacian(50.0, 16) + np.diag(np.full(16, 1e-3))):
        with pytest.raises(ValueError):
            solve._laplacian_spacing(bad)


def test_bench_line_contract():
    """bench.py prints BASELINE.json's metric verbatim and carries every key of the driver's contract plus the
    roofline / cpu_baseline objects (static check: the bench itself needs the GPU)."""
    import json
    import re
    src = open(os.path.join(ROOT, "bench.py"), encoding="utf-8").read()
    metric = re.search(r'"metric": "([^"]+)"', src).group(1)
    assert metric == json.load(open(os.path.join(ROOT, "BASELINE.json"), encoding="utf-8"))["metric"]
    for key in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert f'"{key}"' in src, key
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert f'"{key}"' in src, key
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert f'"{key}"' in src, key
    assert "torch.cuda.Event" not in src           # durations come from HIP events on the library's own stream


def test_header_is_plain_c(tmp_path):
    """include/picstep.h is the contract for ANY FFI (cgo, JNI, ctypes ...): it must compile as C99, and a C caller
    must be able to fill pic_config and take the address of every entry point."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    hdr = os.path.join(ROOT, "include")
    names = sorted(_abi.SIGNATURES)
    src = tmp_path / "use_header.c"
    src.write_text('#include "picstep.h"\n#include <stddef.h>\n'
                   "int main(void) {\n  pic_config cfg = {0};\n  cfg.N = 1000; cfg.Ng = 64; cfg.num_envs = 1; cfg.L = 50.0; cfg.n0 = 1.0; cfg.dt = 0.1;\n"
                   "  cfg.particle_dtype = PIC_F32; cfg.position_dtype = PIC_POS_FIXED32; cfg.accum_dtype = PIC_ACC_AUTO; cfg.interpol = PIC_CIC;\n"
                   "  void* fns[] = {" + ", ".join(f"(void*)&{n}" for n in names) + "};\n"
                   "  return (int)(sizeof(fns) / sizeof(fns[0])) - " + str(len(names)) + " + (int)(sizeof(cfg) != 80);\n}\n")
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-Wno-pedantic", "-I", hdr, "-c", str(src), "-o",
                        str(tmp_path / "use_header.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
