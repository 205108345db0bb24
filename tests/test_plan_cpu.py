"""The launch plan of pic_create (csrc/host_plan.h), pinned on the CPU.

A step's results do not depend on the launch geometry, so no parity test notices a slip in the planner's rules: it
only costs speed.  tests/plan_driver.cpp is the planner as a stand-alone program (host compiler, no HIP, nothing loaded into
Python); this module runs it as a child process over (1) a recorded table with a row on each side of every rule and cap, (2) a
seeded sweep of configurations checked for the invariants the kernels rely on, (3) explicit blocks_per_env.

The rows of TABLE were recorded from the arithmetic as it stood inside pic_create before it moved to host_plan.h (the lines
pasted into a harness, the CU-count query replaced by an argument); that harness and the driver printed the same bytes for the
4 215 981 configurations of the cross product of the threshold values below with both dtypes, both position formats, the four
accumulator settings, both shapes, blocks_per_env in {-1, 0, 1, 7, 122, 65535, 70000} and 256 / 304 CUs.
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimal-control-1d-electrostatic-plasma_amd", "csrc")

# kernel constants (csrc/pic_limits.h)
BLOCK, LDS_LIMIT, SWEEP_STATIC_LDS, RESIDENT_STATIC_LDS = 512, 64 * 1024, (2 * 8 + 2) * 8, (4 * 8 + 4 + 2 * 16) * 8

# a configuration is one line of the driver's input:
FIELDS = "N Ng num_envs particle_dtype position_dtype accum_dtype interpol blocks_per_env placement placement_ms env_index_base L dt n0 ncu"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    args = ["-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "plan_driver.cpp"), "-o", out]
    cxx = shutil.which("c++")
    if cxx:
        cmd = [cxx] + args
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no host C++ compiler (c++ or hipcc) to build tests/plan_driver.cpp with")
        cmd = [hipcc, "-x", "c++"] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        res = p.stdout.splitlines()
        assert len(res) == len(lines)
        return res
    return run


def parse(line):
    assert line.startswith("ok "), line
    d = {}
    for kv in line.split()[1:]:
        k, v = kv.split("=")
        d[k] = float.fromhex(v) if "0x" in v else int(v)
    return d


# (configuration, expected output of the driver), the comment in front says which rule the row pins
TABLE = [
    # bench.py config 1 / BASELINE config 1: streaming (N > 8192) and small: one tile per workgroup
    ('10000 128 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-7 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=10048 fg=48 magic=0x1.8p+4 chunk=1024 nblk=10 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # bench.py config 2, the flagship: 8-tile rule, light inner steps, read-only C, separate v
    ('1000000 256 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # bench.py config 3: fixed-point positions, packed accumulator
    ('1000000 512 128 1 1 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=2 acc_kind=2 esz=4 vec=4 dx=0x1.9p-4 scale=0x1.0c6f7a0b5ed8dp-11 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=16384 nblk=62 S=1 R=1 sweep_lds=10280 sweep_lds_rc=12336 solve_lds=8192 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=26664 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=1'),
    # bench.py config 4: the by10 floor lifts 128 workgroups to 391
    ('4000000 1024 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-5 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=4000000 fg=40 magic=0x1.8p+12 chunk=10240 nblk=391 S=1 R=1 sweep_lds=24624 sweep_lds_rc=32832 solve_lds=16384 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=57392 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=1'),
    # bench.py config 5: by10 floor, float32
    ('10000000 256 128 1 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=1 acc_kind=2 esz=4 vec=4 dx=0x1.9p-3 scale=0x1.ad7f29abcaf49p-16 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=10000000 fg=38 magic=0x1.8p+14 chunk=20480 nblk=489 S=1 R=1 sweep_lds=5160 sweep_lds_rc=6192 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=13352 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # BASELINE N=1e5, Ng=256: small, capped at 64 workgroups, 49 after the chunk rounding
    ('100000 256 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.4f8b588e368f1p-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=100032 fg=45 magic=0x1.8p+7 chunk=2048 nblk=49 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # BASELINE N=1e6, Ng=256, one environment: tiles_min 8 -> 4 and the k loop; S = 4
    ('1000000 256 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=4096 nblk=245 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # the reference's N=5000, Ng=250: resident 8 x 10, carried cells
    ('5000 250 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.999999999999ap-3 scale=0x1.9999999999999p-5 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=6048 sweep_lds_rc=8064 solve_lds=4000 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=14048 res_carry_bytes=102400 h_part_at_create=1 h_fields=1 v_separate=0'),
    # flagship with PIC_PLACE_OFF: v_separate off, nothing else moves
    ('1000000 256 64 0 0 0 0 0 1 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # resident shape at N = 2048: 8 x 4
    ('2048 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1p-4 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=2048 fg=50 magic=0x1.8p+2 chunk=1024 nblk=2 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=4 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # resident shape at N = 2049: 8 x 8
    ('2049 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.ffc007ff002p-5 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=2112 fg=50 magic=0x1.8p+2 chunk=1024 nblk=3 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=8 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # resident shape at N = 4096: 8 x 8
    ('4096 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1p-5 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=4096 fg=49 magic=0x1.8p+3 chunk=1024 nblk=4 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=8 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # resident shape at N = 4097: 8 x 10; fg leaves the clamp (49)
    ('4097 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.ffe001ffe002p-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=4160 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # resident shape at N = 5120: 8 x 10
    ('5120 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.999999999999ap-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5120 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # resident shape at N = 5121: 8 x 16, no carry block
    ('5121 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.99851fbe69adfp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5184 fg=49 magic=0x1.8p+3 chunk=1024 nblk=6 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=16 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # resident shape at N = 8192: 8 x 16
    ('8192 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1p-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=8192 fg=48 magic=0x1.8p+4 chunk=1024 nblk=8 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=16 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # resident shape at N = 8193: none: streaming
    ('8193 128 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.fff0007ffc003p-7 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=8256 fg=48 magic=0x1.8p+4 chunk=1024 nblk=9 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # worth: N <= 5120 is resident with any number of environments
    ('5120 128 31 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.999999999999ap-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5120 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=3174400 h_part_at_create=1 h_fields=1 v_separate=0'),
    # worth: N > 5120 with 31 environments is left to the sweeps
    ('8000 128 31 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.0624dd2f1a9fcp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=8000 fg=49 magic=0x1.8p+3 chunk=1024 nblk=8 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=8 res_ppt=16 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # worth: N > 5120 with 32 environments is resident
    ('8000 128 32 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.0624dd2f1a9fcp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=8000 fg=49 magic=0x1.8p+3 chunk=1024 nblk=8 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=16 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # small: N = 131072 is the last small one (64 workgroups at most)
    ('131072 256 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1p-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=131072 fg=44 magic=0x1.8p+8 chunk=2048 nblk=64 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # small: N = 131073 is not (4 tiles per workgroup)
    ('131073 256 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.ffff00007fffcp-10 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=131136 fg=44 magic=0x1.8p+8 chunk=4096 nblk=33 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # small: N E = 4e6 exactly
    ('125000 256 32 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=125056 fg=45 magic=0x1.8p+7 chunk=2048 nblk=62 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # small: N E just over 4e6
    ('125001 256 32 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6eed4edc98cp-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=125056 fg=45 magic=0x1.8p+7 chunk=8192 nblk=16 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 2
    ('1000000 256 2 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=4096 nblk=245 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 3 (the case the comment names: 3 x 163)
    ('1000000 256 3 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=6144 nblk=163 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 4
    ('1000000 256 4 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 5
    ('1000000 256 5 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=7168 nblk=140 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 6
    ('1000000 256 6 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 8
    ('1000000 256 8 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # k loop at N = 1e6, E = 12
    ('1000000 256 12 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=2 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # S: 16 environments take 2 sub-rows
    ('1000000 256 16 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=2 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # S: 17 environments take 1
    ('1000000 256 17 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # explicit blocks_per_env = 7: fewer than 8 workgroups per sub-row, S = 1
    ('1000000 256 1 0 0 0 0 7 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=143360 nblk=7 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # explicit blocks_per_env = 122: the chunk rounds up to 9 tiles, 109 workgroups
    ('1000000 256 1 0 0 0 0 122 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0c6f7a0b5ed8dp-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=9216 nblk=109 S=4 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # 2^27-byte chunk cap: N = cap fits one workgroup
    ('134216704 256 1 0 0 0 0 1 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.0000800040002p-19 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=134216704 fg=35 magic=0x1.8p+17 chunk=134216704 nblk=1 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # 2^27-byte chunk cap: N = cap + 1 needs two
    ('134216705 256 1 0 0 0 0 1 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.00007fe03fe03p-19 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=134216768 fg=35 magic=0x1.8p+17 chunk=67108864 nblk=2 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # 2^20 packed-count cap: N = cap fits one workgroup
    ('1046528 256 1 1 0 0 0 1 0 0 0 50 0.1 1 256',
     'ok fmt=1 acc_kind=2 esz=4 vec=4 dx=0x1.9p-3 scale=0x1.008040201008p-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1046528 fg=42 magic=0x1.8p+10 chunk=1046528 nblk=1 S=1 R=1 sweep_lds=5160 sweep_lds_rc=6192 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=13352 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # 2^20 packed-count cap: N = cap + 1 needs two
    ('1046529 256 1 1 0 0 0 1 0 0 0 50 0.1 1 256',
     'ok fmt=1 acc_kind=2 esz=4 vec=4 dx=0x1.9p-3 scale=0x1.0080301005018p-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1046592 fg=42 magic=0x1.8p+10 chunk=524288 nblk=2 S=1 R=1 sweep_lds=5160 sweep_lds_rc=6192 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=13352 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # nblk > 65535 from the packed cap at N = 2^36
    ('68719476736 256 1 1 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: blocks_per_env too large'),
    # nblk > 65535 from blocks_per_env = 70000 at N = 2^36
    ('68719476736 256 1 0 0 0 0 70000 0 0 0 50 0.1 1 256',
     'err -1 pic_create: blocks_per_env too large'),
    # fg clamped at 50 (N = 1)
    ('1 4 1 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p+3 scale=0x1p+2 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=64 fg=50 magic=0x1.8p+2 chunk=1024 nblk=1 S=1 R=1 sweep_lds=144 sweep_lds_rc=192 solve_lds=64 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=4 res_R=1 res_lean=0 res_lds=272 res_carry_bytes=40960 h_part_at_create=1 h_fields=1 v_separate=0'),
    # light_inner_steps: float64 state of exactly 256 MB
    ('1048576 256 16 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1p-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1048576 fg=41 magic=0x1.8p+11 chunk=8192 nblk=128 S=2 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # light_inner_steps: float64 state one row of 64 below 256 MB
    ('1048512 256 16 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.00040010004p-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1048512 fg=42 magic=0x1.8p+10 chunk=8192 nblk=128 S=2 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # light_inner_steps: float32 state of exactly 256 MB
    ('1048576 256 32 1 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=1 acc_kind=2 esz=4 vec=4 dx=0x1.9p-3 scale=0x1p-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1048576 fg=41 magic=0x1.8p+11 chunk=16384 nblk=64 S=1 R=1 sweep_lds=5160 sweep_lds_rc=6192 solve_lds=4096 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=13352 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=1'),
    # light_inner_steps: float32 state just below
    ('1048512 256 32 1 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=1 acc_kind=2 esz=4 vec=4 dx=0x1.9p-3 scale=0x1.00040010004p-12 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1048512 fg=42 magic=0x1.8p+10 chunk=16384 nblk=64 S=1 R=1 sweep_lds=5160 sweep_lds_rc=6192 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=13352 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # sweep_lds_rc: float64 Ng = 2041 is the last mesh with room for the second field tile
    ('1000000 2041 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.915f334ce346ep-6 scale=0x1.0b84988094e5dp-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=1 R=1 sweep_lds=49032 sweep_lds_rc=65376 solve_lds=32656 light_inner_steps=1 readonly_auto=1 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=114344 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=1'),
    # sweep_lds_rc: float64 Ng = 2042 has none, readonly_auto goes off
    ('1000000 2042 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.912ce1a93eef3p-6 scale=0x1.0ba6266fd651bp-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=1 R=1 sweep_lds=49056 sweep_lds_rc=0 solve_lds=32672 light_inner_steps=1 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=114400 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=1'),
    # Ng too large, sweeps: float64 Ng = 2722 is the last that fits
    ('1000000 2722 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.2cf486ad6ce88p-6 scale=0x1.64c729f59ccfbp-9 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=1000000 fg=42 magic=0x1.8p+10 chunk=8192 nblk=123 S=1 R=1 sweep_lds=65376 sweep_lds_rc=0 solve_lds=43552 light_inner_steps=1 readonly_auto=0 resident=0 res_nw=0 res_ppt=0 res_R=1 res_lean=0 res_lds=152480 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=1'),
    # Ng too large, sweeps: float64 Ng = 2723
    ('1000000 2723 64 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: Ng too large for the LDS-resident mesh (at most 2722 cells with this particle dtype)'),
    # resident or fail: float64 Ng = 1159 is the last that fits
    ('5000 1159 4 0 0 0 0 -1 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.616879ed011acp-5 scale=0x1.dab9f559b3d07p-3 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=27864 sweep_lds_rc=37152 solve_lds=18544 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=64952 res_carry_bytes=409600 h_part_at_create=1 h_fields=1 v_separate=0'),
    # resident or fail: float64 Ng = 1160, with the computed limit
    ('5000 1160 4 0 0 0 0 -1 0 0 0 50 0.1 1 256',
     'err -1 pic_create: the resident schedule needs N <= 8192, Ng <= 1159 (this particle dtype) and an integer accumulator'),
    # resident or fail: N = 8193
    ('8193 128 4 0 0 0 0 -1 0 0 0 50 0.1 1 256',
     'err -1 pic_create: the resident schedule needs N <= 8192, Ng <= 1159 (this particle dtype) and an integer accumulator'),
    # resident or fail: float64 accumulator
    ('5000 128 4 0 0 3 0 -1 0 0 0 50 0.1 1 256',
     'err -1 pic_create: the resident schedule needs N <= 8192, Ng <= 1159 (this particle dtype) and an integer accumulator'),
    # res_lean: 256 environments on 256 CUs keep the carrying kernel
    ('5000 128 256 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # res_lean: 257 environments on 256 CUs run lean
    ('5000 128 257 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=1 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=0'),
    # res_lean: 257 environments on 304 CUs do not
    ('5000 128 257 0 0 0 0 0 0 0 0 50 0.1 1 304',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=0'),
    # res_lean: more environments than CUs but 16 per lane: not lean
    ('8192 128 257 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1p-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=8192 fg=48 magic=0x1.8p+4 chunk=1024 nblk=8 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=16 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=0'),
    # res_lean: TSC with 16 per lane
    ('8192 128 64 0 0 0 1 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1p-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=8192 fg=48 magic=0x1.8p+4 chunk=1024 nblk=8 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=16 res_R=1 res_lean=1 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # res_lean: TSC with 10 per lane is not
    ('5120 128 64 0 0 0 1 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.999999999999ap-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5120 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # carry block: 10 per lane, float64, 32 environments
    ('5000 128 32 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=3276800 h_part_at_create=1 h_fields=1 v_separate=0'),
    # carry block: 33 environments have none
    ('5000 128 33 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=3120 sweep_lds_rc=4160 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=7216 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # carry block: float32 has none
    ('5000 128 4 1 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=1 acc_kind=2 esz=4 vec=4 dx=0x1.9p-2 scale=0x1.a36e2eb1c432dp-6 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=2048 nblk=3 S=1 R=1 sweep_lds=2600 sweep_lds_rc=3120 solve_lds=2048 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=6696 res_carry_bytes=0 h_part_at_create=1 h_fields=1 v_separate=0'),
    # h_fields: meshes of exactly 256 KB
    ('5000 256 128 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.9p-3 scale=0x1.a36e2eb1c432dp-5 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=6192 sweep_lds_rc=8256 solve_lds=4096 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=14384 res_carry_bytes=0 h_part_at_create=0 h_fields=1 v_separate=0'),
    # h_fields: one cell more
    ('5000 257 128 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'ok fmt=0 acc_kind=1 esz=8 vec=2 dx=0x1.8e718e718e719p-3 scale=0x1.a5119ce075f7p-5 cs0=0x1.59e8b6eb96339p-1 cs1=-0x1.67a2dbae58cep-3 cs2=-0x1.67a2dbae58cep-3 cs3=0x1.59e8b6eb96339p-1 ds0=0x0p+0 ds1=0x1.59e8b6eb96339p+0 ds2=-0x1.b3d16dd72c671p+0 ds3=0x1.59e8b6eb96339p+0 ld=5056 fg=49 magic=0x1.8p+3 chunk=1024 nblk=5 S=1 R=1 sweep_lds=6216 sweep_lds_rc=8288 solve_lds=4112 light_inner_steps=0 readonly_auto=0 resident=1 res_nw=8 res_ppt=10 res_R=1 res_lean=0 res_lds=14440 res_carry_bytes=0 h_part_at_create=0 h_fields=0 v_separate=0'),
    # check_config: N < 1
    ('0 250 4 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: need N>=1, Ng>=4, num_envs>=1, L>0, dt>0, n0>0'),
    # check_config: Ng < 4
    ('5000 3 4 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: need N>=1, Ng>=4, num_envs>=1, L>0, dt>0, n0>0'),
    # check_config: N > 2^36
    ('68719476737 250 4 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: N > 2^36'),
    # check_config: num_envs > 65535
    ('5000 250 65536 0 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: num_envs > 65535'),
    # check_config: env_index_base < 0
    ('5000 250 4 0 0 0 0 0 0 0 -1 50 0.1 1 256',
     'err -1 pic_create: env_index_base < 0'),
    # check_config: particle_dtype
    ('5000 250 4 2 0 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: particle_dtype must be PIC_F64 or PIC_F32'),
    # check_config: position_dtype
    ('5000 250 4 0 2 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: position_dtype must be PIC_POS_FLOAT or PIC_POS_FIXED32'),
    # check_config: fixed32 with float64
    ('5000 250 4 0 1 0 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: 32-bit fixed-point positions go with float32 particles'),
    # check_config: accum_dtype
    ('5000 250 4 0 0 4 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: accum_dtype must be PIC_ACC_AUTO, _FIX64, _PACKED or _F64'),
    # check_config: interpol
    ('5000 250 4 0 0 0 2 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: interpol must be PIC_CIC or PIC_TSC'),
    # check_config: packed with float64
    ('5000 250 4 0 0 2 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: the packed accumulator needs float32 particles'),
    # check_config: packed with TSC
    ('5000 250 4 1 0 2 1 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: the packed accumulator is CIC only'),
    # check_config: placement
    ('5000 250 4 0 0 0 0 0 2 0 0 50 0.1 1 256',
     'err -1 pic_create: placement must be PIC_PLACE_AUTO or PIC_PLACE_OFF'),
    # check_config: placement_ms < 0
    ('5000 250 4 0 0 0 0 0 0 -1 0 50 0.1 1 256',
     'err -1 pic_create: placement_ms < 0'),
    # check_config: float64 accumulator with float32
    ('5000 250 4 1 0 3 0 0 0 0 0 50 0.1 1 256',
     'err -1 pic_create: the float64 accumulator needs float64 particles'),
]


def test_recorded_plans(driver):
    assert len(TABLE) <= 80
    got = driver([cfg for cfg, _ in TABLE])
    for (cfg, want), have in zip(TABLE, got):
        assert have == want, cfg


def random_configs(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        pd = rng.randint(0, 1)
        pos = rng.randint(0, 1) if pd else 0
        sh = rng.randint(0, 1)
        acc = rng.choice([0, 1, 2] if pd and not sh else [0, 1] if pd else [0, 1, 3])
        N = min(1 << 36, int(2 ** rng.uniform(0, 36.2)) + rng.choice([0, 0, 1, 63]))
        E = min(65535, int(2 ** rng.uniform(0, 16.1)))
        Ng = rng.choice([4, 128, 250, 256, 512, 1024, rng.randint(4, 3300)])
        bpe = rng.choice([0, 0, 0, -1, 1, 7, 122, rng.randint(1, 70000)])
        out.append(f"{N} {Ng} {E} {pd} {pos} {acc} {sh} {bpe} {rng.randint(0, 1)} 0 0 50 0.1 1 {rng.choice([64, 256, 304])}")
    return out


def test_plan_invariants(driver):
    """What the kernels rely on, for every accepted configuration of a seeded sweep."""
    cfgs = random_configs(4000, 20240607)
    res = driver(cfgs)
    accepted = 0
    for cfg, line in zip(cfgs, res):
        if line.startswith("err "):
            continue
        accepted += 1
        c = dict(zip(FIELDS.split(), cfg.split()))
        N, p = int(c["N"]), parse(line)
        assert p["chunk"] % (BLOCK * p["vec"]) == 0, cfg
        assert (p["nblk"] - 1) * p["chunk"] < N <= p["nblk"] * p["chunk"], cfg
        assert 1 <= p["nblk"] <= 65535, cfg
        assert p["chunk"] * p["esz"] < 2 ** 31, cfg
        if p["acc_kind"] == 2:
            assert p["chunk"] < 2 ** 20, cfg
        assert p["sweep_lds"] + SWEEP_STATIC_LDS <= LDS_LIMIT, cfg
        assert p["sweep_lds_rc"] == 0 or p["sweep_lds_rc"] + SWEEP_STATIC_LDS <= LDS_LIMIT, cfg
        if p["resident"]:
            assert p["res_lds"] + RESIDENT_STATIC_LDS <= LDS_LIMIT, cfg
            assert N <= p["res_nw"] * 64 * p["res_ppt"], cfg
    assert accepted > 1000, accepted


def test_explicit_blocks_per_env(driver):
    """blocks_per_env > 0 is honoured up to the two caps: the same nblk follows from the chunk rounding alone."""
    cfgs = [c for c in random_configs(6000, 7) if int(c.split()[7]) > 0]
    checked = 0
    for cfg, line in zip(cfgs, driver(cfgs)):
        if line.startswith("err "):
            continue
        c = dict(zip(FIELDS.split(), cfg.split()))
        N, p = int(c["N"]), parse(line)
        tile = BLOCK * p["vec"]
        nb = int(c["blocks_per_env"])
        caps = [(1 << 27) - tile] + ([(1 << 20) - tile] if p["acc_kind"] == 2 else [])
        for cap in caps:
            nb = max(nb, -(-N // cap))
        chunk = -(-(-(-N // nb)) // tile) * tile
        assert (p["chunk"], p["nblk"]) == (chunk, -(-N // chunk)), cfg
        assert not p["resident"], cfg
        checked += 1
    assert checked > 500, checked
