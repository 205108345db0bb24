"""The step schedule with CallShape::alternate_stores (csrc/host_schedule.h), pinned on the CPU.

Inside a call of two or more whole Yoshida-4 steps with the read-only sweep C in force and no feedback law, every second inner
step (a Y step: B2_RO, C_RB, D2_RO) stores its particles once and the X step behind it opens with B2_RD.
tests/schedule_alt_driver.cpp is tests/schedule_driver.cpp with the flag as a fourth header field and an op `tB` that sets it;
this module runs it as a child process and holds its output to the ring's invariants of tests/test_schedule_cpu.py (the same
checker), to the rules of the two kinds of step, to the count of storing sweeps and to a small recorded table.
"""
import os
import random
import shutil
import subprocess

import pytest

from test_schedule_cpu import CSRC, KIND, KIND_NAMES, OPS, ROOT, check, tree

ST_A, ST_B2, ST_C_RO, ST_D_RC, ST_D2_RC, ST_B2_RO, ST_C_RB, ST_D2_RO, ST_B2_RD = 0, 6, 12, 13, 14, 15, 16, 17, 18
KIND_ALT = {**KIND, ST_B2_RO: 1, ST_C_RB: 2, ST_D2_RO: 3, ST_B2_RD: 1}   # the profile kinds of the new stages
NEW = (ST_B2_RO, ST_C_RB, ST_D2_RO, ST_B2_RD)
PUSH_NO_STORE = (ST_A, ST_C_RO, ST_B2_RO, ST_D2_RO)                              # push sweeps that store no particles
READER = {ST_C_RO: (ST_D_RC, ST_D2_RC), ST_B2_RO: (ST_C_RB,), ST_D2_RO: (ST_B2_RD,)}   # who reads the tile a sweep leaves in e2
NO_SWEEP = (-1, 4, 5)                                                            # a solve, REFRESH, PROBE


def _build(tmp, name):
    out = str(tmp / name)
    args = ["-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", out]
    cxx = shutil.which("c++")
    if cxx:
        cmd = [cxx] + args
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no host C++ compiler (c++ or hipcc) to build tests/%s.cpp with" % name)
        cmd = [hipcc, "-x", "c++"] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(scripts):
        p = subprocess.run([out], input="".join(s + "\n" for s in scripts), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return p.stdout
    return run


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("schedule_alt")
    return _build(tmp, "schedule_alt_driver"), _build(tmp, "schedule_driver")


def calls(lines):
    """(script, op, [launch fields]) for every op of the driver's output; `[` and `]` lines are skipped (a walk's ops stand alone)."""
    script, op, out = None, None, []
    for line in lines:
        tag = line[0]
        if tag == "B":
            script = line[:100]
        elif tag == "O":
            op = line.split()[1]
            out.append((script, op, []))
        elif tag == "L" and not line.startswith("L unclean"):
            out[-1][2].append(line.split())
    return out


def check_alt(lines):
    """The rules of the two kinds of step, for every call of the output.  Returns the number of calls that held a Y step."""
    with_y = 0
    for script, op, ls in calls(lines):
        stages = [int(f[1]) for f in ls]
        sweeps = [s for s in stages if s not in NO_SWEEP]
        # a sweep that leaves its tile in e2 is directly followed by the launch that reads it, and nothing else reads one
        for k, s in enumerate(stages):
            if s in READER:
                assert k + 1 < len(stages) and stages[k + 1] in READER[s], (script, op, stages)
            for w, rs in READER.items():
                if s in rs:
                    assert k > 0 and stages[k - 1] == w, (script, op, stages)
        # no two consecutive push sweeps store nothing: what the plan yields (a sweep A is followed by the first step's B, C_RO by
        # a D that stores, B2_RO by C_RB, D2_RO by B2_RD): the particles in memory are never more than one sweep behind
        for a, b in zip(sweeps, sweeps[1:]):
            assert not (a in PUSH_NO_STORE and b in PUSH_NO_STORE), (script, op, stages)
        if not any(s in NEW for s in stages):
            continue
        with_y += 1
        assert op[0] in "sepha" and int(op[1:]) >= 3, (script, op, stages)          # (a call of two steps has no Y step)
        K = int(op[1:])
        by_step = {}
        for f in ls:
            if int(f[1]) not in NO_SWEEP and int(f[1]) != ST_A:
                by_step.setdefault(int(f[17]), []).append(int(f[1]))
        assert sorted(by_step) == list(range(K)), (script, op, stages)
        for i in range(K):
            y = i >= 1 and (K - 1 - i) % 2 == 1
            b, c, d = by_step[i]
            if y:
                assert (b, c, d) == (ST_B2_RO, ST_C_RB, ST_D2_RO), (script, op, i, by_step)
            else:
                after_y = i >= 2 and (K - 1 - (i - 1)) % 2 == 1
                assert b == (ST_B2_RD if after_y else 1 if i == 0 else ST_B2), (script, op, i, by_step)
                assert c == ST_C_RO and d == (ST_D_RC if i == K - 1 else ST_D2_RC), (script, op, i, by_step)
        assert by_step[0][0] == 1 and by_step[K - 1][2] == ST_D_RC                  # the first and the last step are X
        # a re-deriving sweep carries the drift of the sub-stage it repeats in c_prev: c2 in C_RB (sweep B's), c4 in B2_RD (sweep D's)
        for f in ls:
            if int(f[1]) == ST_C_RB:
                assert f[2] == "-0x1.67a2dbae58cep-3", (script, op, f)
            if int(f[1]) == ST_B2_RD:
                assert f[2] == "0x1.59e8b6eb96339p-1", (script, op, f)
    return with_y


def storing(ls):
    return sum(1 for f in ls if int(f[1]) not in NO_SWEEP and int(f[1]) not in PUSH_NO_STORE)


def test_store_count(drivers):
    """K steps in one call: 2 K - floor((K - 1) / 2) storing sweeps with the mode on (2 K without), on a small state and a large."""
    alt, _ = drivers
    for light in (0, 1):
        for op in "sepha":
            out = alt(["0 %d 1 %d r %s%d" % (light, flag, op, K) for flag in (1, 0) for K in range(1, 14)])
            got = [storing(ls) for _, o, ls in calls(out.splitlines()) if o[0] == op]
            assert got[:13] == [2 * K - (K - 1) // 2 for K in range(1, 14)], (light, op, got)
            assert got[13:] == [2 * K for K in range(1, 14)], (light, op, got)
            assert check(out.splitlines()) == 26


def test_fallbacks_give_the_old_descriptors(drivers):
    """A feedback call, a staged step, nsteps == 1, another integrator and readonly_c off: the flag changes no descriptor; and
    with the flag off the new driver prints what tests/schedule_driver.cpp prints."""
    alt, old = drivers
    scripts = ["0 1 1 r f4 f1 s1 g g g s1 e1 a1 h1 p1", "0 0 1 i f3 s1 g s1", "0 1 0 r s4 a5 h3 e6 p4 g g g s3", "0 0 0 r s5 a4",
               "1 1 1 r s4 e3", "2 1 1 r s4 p3 s5", "3 0 1 r s3 s4", "0 1 1 r o0 s4 a5", "2 1 1 r s3 k0 s1 f3"]

    def with_flag(s, flag):
        f = s.split()
        return " ".join(f[:3] + [str(flag)] + f[3:])

    def body(text):
        return [line for line in text.splitlines() if line[0] != "B"]

    on, off, was = alt([with_flag(s, 1) for s in scripts]), alt([with_flag(s, 0) for s in scripts]), old(scripts)
    assert body(on) == body(off) == body(was)
    assert check_alt(on.splitlines()) == 0
    # ... and every script of the old module's wider alphabet, flag off
    rng = random.Random(7)
    ops = OPS + ["s7", "f1", "f3", "e3", "p3", "h2", "h3", "a2", "a3", "a4", "k0", "k1", "k2", "k3", "o0", "o1"]
    more = ["%d %d %d " % (rng.randrange(4), rng.randrange(2), rng.randrange(2)) + " ".join(rng.choice(ops) for _ in range(12))
            for _ in range(300)]
    assert body(alt([with_flag(s, 0) for s in more])) == body(old(more))


def test_every_order_to_depth_4(drivers):
    """tests/test_schedule_cpu.py's walk of every order of its nine operations to depth 4, flag on: Yoshida-4, a single-sweep scheme
    and Verlet, with and without the light path and read-only C."""
    alt, _ = drivers
    walk = tree(OPS, 4)
    scripts = ["%d %d %d 1%s" % (scheme, light, ro, walk) for scheme in (0, 1, 2) for light in (0, 1) for ro in (0, 1)]
    lines = alt(scripts).splitlines()
    assert check(lines) == 12
    assert check_alt(lines) > 1000          # (s3 and s4 under Yoshida-4 with read-only C hold a Y step)


def test_random_scripts(drivers):
    """A seeded sweep: 4000 scripts of 12 operations from the wider alphabet, longer calls and the two mode setters included."""
    alt, _ = drivers
    rng = random.Random(20250301)
    ops = OPS + ["s5", "s6", "s7", "s9", "f1", "f3", "e3", "e4", "p3", "p6", "h2", "h3", "h5", "a2", "a3", "a4", "a7", "k0", "k0", "k1", "k2",
                 "k3", "o0", "o1", "o1", "t0", "t1", "t1"]
    scripts = ["%d %d %d %d " % (rng.randrange(4), rng.randrange(2), rng.randrange(2), rng.randrange(2)) +
               " ".join(rng.choice(ops) for _ in range(12)) for _ in range(4000)]
    lines = alt(scripts).splitlines()
    assert check(lines) == 4000
    assert check_alt(lines) > 1000


def test_gpu_script_launch_counts(drivers):
    """The launches per profile kind of the script tests/test_gpu_alternate_stores.py::test_alternate_launches_match_schedule runs
    on the device: the counts written there are these."""
    alt, _ = drivers
    counts = [0] * 8
    for _, _, ls in calls(alt(["0 0 1 1 i r s1 s5 s4"]).splitlines()):
        for f in ls:
            counts[KIND_ALT[int(f[1])]] += 1
    assert dict(zip(KIND_NAMES, counts)) == {"sweep_A": 0, "sweep_B": 10, "sweep_C": 10, "sweep_D": 10, "field_solve": 4, "sweep_aux": 1,
                                             "resident": 0, "sweep_integrator": 0}


# The sweeps of `r sK` with read-only C and the mode on, K = 2 ... 5 (the refresh in front: row 6 holds q1, rows 0 ... 5 are clean):
#   stage c_prev in fill0 fill1 post reverse step post_step
C1, C3, C4 = "0x1.59e8b6eb96339p-1", "-0x1.67a2dbae58cep-3", "0x1.59e8b6eb96339p-1"       # c1, c2 = c3, c4 = c1
B_FIRST = "1 %s 6 5 -1 -1" % C1
TABLE = {
    2: ["1 %s 6 5 -1 -1 1 0 -1" % C1, "12 0x0p+0 5 7 -1 -1 0 0 -1", "14 %s 7 -1 6 -1 1 0 -1" % C3,
        "6 %s 6 5 4 -1 0 1 -1" % C1, "12 0x0p+0 5 7 -1 4 1 1 0", "13 %s 7 6 3 -1 0 1 -1" % C3],
    3: ["1 %s 6 5 -1 -1 1 0 -1" % C1, "12 0x0p+0 5 7 -1 -1 0 0 -1", "14 %s 7 -1 6 -1 1 0 -1" % C3,
        "15 %s 6 5 4 -1 0 1 -1" % C1, "16 %s 5 7 -1 4 1 1 0" % C3, "17 0x0p+0 7 -1 6 -1 0 1 -1",
        "18 %s 6 5 4 -1 1 2 -1" % C4, "12 0x0p+0 5 7 -1 4 0 2 1", "13 %s 7 6 3 -1 1 2 -1" % C3],
    4: ["1 %s 6 5 -1 -1 1 0 -1" % C1, "12 0x0p+0 5 7 -1 -1 0 0 -1", "14 %s 7 -1 6 -1 1 0 -1" % C3,
        "6 %s 6 5 4 -1 0 1 -1" % C1, "12 0x0p+0 5 7 -1 4 1 1 0", "14 %s 7 -1 6 -1 0 1 -1" % C3,
        "15 %s 6 5 4 -1 1 2 -1" % C1, "16 %s 5 7 -1 4 0 2 1" % C3, "17 0x0p+0 7 -1 6 -1 1 2 -1",
        "18 %s 6 5 4 -1 0 3 -1" % C4, "12 0x0p+0 5 7 -1 4 1 3 2", "13 %s 7 6 3 -1 0 3 -1" % C3],
    5: ["1 %s 6 5 -1 -1 1 0 -1" % C1, "12 0x0p+0 5 7 -1 -1 0 0 -1", "14 %s 7 -1 6 -1 1 0 -1" % C3,
        "15 %s 6 5 4 -1 0 1 -1" % C1, "16 %s 5 7 -1 4 1 1 0" % C3, "17 0x0p+0 7 -1 6 -1 0 1 -1",
        "18 %s 6 5 4 -1 1 2 -1" % C4, "12 0x0p+0 5 7 -1 4 0 2 1", "14 %s 7 -1 6 -1 1 2 -1" % C3,
        "15 %s 6 5 4 -1 0 3 -1" % C1, "16 %s 5 7 -1 4 1 3 2" % C3, "17 0x0p+0 7 -1 6 -1 0 3 -1",
        "18 %s 6 5 4 -1 1 4 -1" % C4, "12 0x0p+0 5 7 -1 4 0 4 3", "13 %s 7 6 3 -1 1 4 -1" % C3],
}


@pytest.mark.parametrize("K", sorted(TABLE))
def test_table(drivers, K):
    alt, _ = drivers
    for light in (0, 1):                     # (while the mode is in force a small state plans its inner steps as a large one does)
        out = alt(["0 %d 1 1 r s%d" % (light, K)]).splitlines()
        (_, _, refresh), (_, op, ls) = calls(out)
        assert op == "s%d" % K and [int(f[1]) for f in refresh] == [4, -1]
        got = [" ".join([f[1], f[2], f[5], f[6], f[7], f[9], f[12], f[17], f[18]]) for f in ls if int(f[1]) != -1]
        assert got == TABLE[K], (light, got)
        assert [int(f[1]) for f in ls].count(-1) == 1 and int(ls[-1][1]) == -1      # one solve launch, behind the last sweep
