"""The table of sweep stages (csrc/pic_limits.h: stage_traits) and the schedule's d_prev (csrc/host_schedule.h), pinned on the CPU.

sweep_kernel, push_one, the launch and the step schedule take what a stage is from one constexpr table.  tests/stage_traits_driver.cpp
prints its 19 rows, what follows from each, and the `stage c_prev d_prev` of every launch of three planned calls; this module holds
the rows to a table written out here from the documented meaning of each stage, to the restatements the other schedule tests
already keep (imported, not copied), and d_prev to the Yoshida-4 coefficients of the reference's expressions.
"""
import pytest

from test_schedule_cpu import KIND, NOT_PUSH
from test_schedule_alt_cpu import KIND_ALT, NO_SWEEP, PUSH_NO_STORE, READER, _build

NAMES = ("A", "B", "C", "D", "REFRESH", "PROBE", "B2", "D2", "SE", "FE", "VK", "VM", "C_RO", "D_RC", "D2_RC", "B2_RO", "C_RB", "D2_RO", "B2_RD")
A, B, C, D, REFRESH, PROBE, SCHEME, NONE = 0, 1, 2, 3, 4, 5, 6, -1        # Arith: the arithmetic a stage runs / re-derives
INPUT, NEXT_Q1 = 1, 2                                                      # Mesh2: what the second LDS mesh receives (0: nothing)
COLUMNS = ("arith", "rederives", "stores", "first", "second", "gathers", "reads_v", "pushes", "reads_tile", "leaves_tile",
           "wrap_only", "ends_step", "carries_solve", "kind")
# One row per stage, by hand from what the stage is documented to do:
#           arith  rederives stores first second | gathers reads_v pushes reads_tile leaves_tile wrap_only ends_step carries kind
EXPECTED = {
    "A":       (A,       NONE, 0, 1, 0,        0, 1, 1, 0, 0, 0, 0, 0, 0),    # drift, deposit; reads x and v, stores nothing, solves no field
    "B":       (B,       NONE, 1, 1, 0,        1, 1, 1, 0, 0, 0, 0, 0, 1),
    "C":       (C,       NONE, 1, 1, 0,        1, 1, 1, 0, 0, 0, 0, 1, 2),    # a sweep C may carry the previous step's solve
    "D":       (D,       NONE, 1, 1, NEXT_Q1,  1, 1, 1, 0, 0, 0, 1, 0, 3),    # ends the step: KE, and the next step's q1 into the second mesh
    "REFRESH": (REFRESH, NONE, 1, 1, NEXT_Q1,  0, 1, 0, 0, 0, 0, 1, 0, 5),    # stores the wrapped x alone; no push, no field
    "PROBE":   (PROBE,   NONE, 0, 1, 0,        0, 0, 0, 0, 0, 0, 0, 0, 5),    # deposits a scratch array: no v
    "B2":      (B,       NONE, 1, 1, INPUT,    1, 1, 1, 0, 0, 0, 0, 0, 1),    # B, and its input positions into the second mesh
    "D2":      (D,       NONE, 1, 0, NEXT_Q1,  1, 1, 1, 0, 0, 1, 1, 0, 3),    # D without the deposit of x': the wrap alone
    "SE":      (SCHEME,  NONE, 1, 1, 0,        1, 1, 1, 0, 0, 0, 1, 0, 7),
    "FE":      (SCHEME,  NONE, 1, 1, 0,        1, 1, 1, 0, 0, 0, 1, 0, 7),
    "VK":      (SCHEME,  NONE, 1, 0, 0,        1, 1, 1, 0, 0, 0, 1, 0, 7),    # the closing half-kick: no deposit
    "VM":      (SCHEME,  NONE, 1, 1, 0,        1, 1, 1, 0, 0, 0, 1, 0, 7),
    "C_RO":    (C,       NONE, 0, 1, 0,        1, 1, 1, 0, 1, 0, 0, 1, 2),    # C without the stores: leaves its field tile
    "D_RC":    (D,       C,    1, 1, NEXT_Q1,  1, 1, 1, 1, 0, 0, 1, 0, 3),    # C again from that tile, then D
    "D2_RC":   (D,       C,    1, 0, NEXT_Q1,  1, 1, 1, 1, 0, 1, 1, 0, 3),    # ... then D2
    "B2_RO":   (B,       NONE, 0, 1, INPUT,    1, 1, 1, 0, 1, 0, 0, 0, 1),    # B2 without the stores
    "C_RB":    (C,       B,    1, 1, 0,        1, 1, 1, 1, 0, 0, 0, 1, 2),    # B again, then C
    "D2_RO":   (D,       NONE, 0, 0, NEXT_Q1,  1, 1, 1, 0, 1, 1, 1, 0, 3),    # D2 without the stores
    "B2_RD":   (B,       D,    1, 1, INPUT,    1, 1, 1, 1, 0, 0, 0, 0, 1),    # D again, then B2
}

# Yoshida-4's coefficients with the reference's expressions (src/env/integration.py:62-69)
PHI = 2 ** (1 / 3)
W0 = (-1) * PHI / (2 - PHI)
W1 = 1 / (2 - PHI)
CS = (0.5 * W1, 0.5 * (W0 + W1), 0.5 * (W0 + W1), 0.5 * W1)
DS = (0.0, W1, W0, W1)


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("stage_traits"), "stage_traits_driver")([]).splitlines()


@pytest.fixture(scope="module")
def rows(output):
    got = {}
    for line in output:
        if line[0] == "T":
            f = [int(w) for w in line.split()[1:]]
            got[f[0]] = dict(zip(COLUMNS, f[1:]))
            assert len(f) == 1 + len(COLUMNS), line
    return got


def test_rows(rows):
    assert sorted(rows) == list(range(19))
    for s, name in enumerate(NAMES):
        assert rows[s] == dict(zip(COLUMNS, EXPECTED[name])), (s, name)


def test_rows_match_the_suite(rows):
    """... and the facts the schedule tests restate by hand."""
    assert {s: r["kind"] for s, r in rows.items()} == {s: k for s, k in KIND_ALT.items() if s != -1}
    assert all(rows[s]["kind"] == k for s, k in KIND.items() if s != -1)
    assert {s for s, r in rows.items() if not r["pushes"]} == set(NOT_PUSH) - {-1} == set(NO_SWEEP) - {-1}
    assert {s for s, r in rows.items() if r["pushes"] and not r["stores"]} == set(PUSH_NO_STORE)
    assert {s for s, r in rows.items() if r["leaves_tile"]} == set(READER)
    assert {s for s, r in rows.items() if r["reads_tile"]} == {s for rs in READER.values() for s in rs}
    for writer, readers in READER.items():                  # a reader re-derives the arithmetic of the sweep whose tile it reads
        for s in readers:
            assert rows[s]["rederives"] == rows[writer]["arith"], (writer, s)
    for s, r in rows.items():                               # what sweep_kernel relies on
        assert not (r["leaves_tile"] and r["reads_tile"]) and (r["stores"] or not r["reads_tile"]), s
        assert r["second"] == (INPUT if NAMES[s].startswith("B2") else NEXT_Q1 if r["arith"] in (D, REFRESH) else 0), s


X_FIRST, X_INNER, X_AFTER_Y, X_LAST, Y = [1, 12, 14], [6, 12, 14], [18, 12, 14], [18, 12, 13], [15, 16, 17]
STAGES = {   # `r s7` on a large state: (readonly_c, alternate_stores) -> the launches of the call (steps 1, 3 and 5 of 0 .. 6 are Y steps)
    (1, 1): X_FIRST + Y + X_AFTER_Y + Y + X_AFTER_Y + Y + X_LAST + [-1],
    (1, 0): X_FIRST + 5 * X_INNER + [6, 12, 13, -1],
    (0, 0): [1, 2, 7] + 5 * [6, 2, 7] + [6, 2, 3, -1],
}
# by stage: (c_prev, d_prev).  c_prev is c1 in a sweep B (its own first drift), else the drift of the re-derived sub-stage; d_prev is
# that sub-stage's kick: d3 = w0 behind C_RO, d2 = w1 in C_RB, d4 = w1 in B2_RD; zero wherever nothing is re-derived
COEFF = {1: (CS[0], 0.0), 6: (CS[0], 0.0), 15: (CS[0], 0.0), 18: (CS[3], DS[3]), 16: (CS[1], DS[1]), 13: (CS[2], DS[2]), 14: (CS[2], DS[2])}


def test_d_prev(output, rows):
    assert (W1.hex(), W0.hex()) == ("0x1.59e8b6eb96339p+0", "-0x1.b3d16dd72c671p+0")     # (d_cur of sweeps B and C in the recorded tables)
    assert DS[2] != DS[1] == DS[3]
    calls = {}
    for line in output:
        f = line.split()
        if f[0] == "C":
            cur = calls.setdefault((int(f[1]), int(f[2])), [])
        elif f[0] == "L":
            cur.append((int(f[1]), float.fromhex(f[2]), float.fromhex(f[3])))
    assert sorted(calls) == sorted(STAGES)
    for mode, ls in calls.items():
        assert [s for s, _, _ in ls] == STAGES[mode], mode
        for s, c_prev, d_prev in ls:
            assert (c_prev, d_prev) == COEFF.get(s, (0.0, 0.0)), (mode, s, c_prev.hex(), d_prev.hex())
            assert (d_prev != 0.0) == (s >= 0 and rows[s]["reads_tile"] == 1), (mode, s)
