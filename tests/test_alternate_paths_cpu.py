"""The calls of tests/test_gpu_alternate_paths.py, cut into parts on the CPU.

`advance()` (csrc/picstep.hip) cuts a stepping call at every recorded step and at every checkpoint step of an open tape, and into
single steps under a tape with a KL or a moments trace; each part is a `plan_call` of its own, with its own X / Y pattern.  A
part of fewer than three steps holds no Y step (B2_RO, C_RB, D2_RO), so a GPU test whose parts never reach three steps says
nothing about the alternate stores.  `parts` restates the cut rule, the tables below are the calls the GPU tests make (that
module imports them from here), and tests/schedule_alt_driver.cpp plans the part sequences with the flag on: the Y steps stand
exactly where the tables say.
"""
import math

import pytest

from test_schedule_alt_cpu import _build, calls, check_alt
from test_schedule_cpu import check


def parts(nsteps, rec_k=0, stride=0, tape_steps=0, every=0, per_step=False):
    """The parts `advance()` cuts a call of nsteps into.  rec_k: steps the recorder has counted so far, stride: its stride
    (0: not recording); tape_steps: steps on the open tape so far, every: its resolved checkpoint interval (0: no tape);
    per_step: the tape records a KL or a moments trace."""
    out, done = [], 0
    while done < nsteps:
        n = nsteps - done
        if stride:
            n = min(n, stride - (rec_k + done) % stride)
        if every:
            n = min(n, every - (tape_steps + done) % every)
        if every and per_step:
            n = 1
        out.append(n)
        done += n
    return out


def resolved_every(max_steps, checkpoint_every):
    """pic_tape_start's interval without a budget: about sqrt(max_steps) for 0, never more than max_steps."""
    every = checkpoint_every or min(max_steps, max(1, math.ceil(math.sqrt(max_steps))))
    return min(every, max_steps)


def call_sequence(seq, stride=0, every=0, per_step=False):
    """[(op, [parts])] for a sequence of calls [(driver op letter, nsteps)] on one handle: the recorder and the tape count on."""
    out, k = [], 0
    for op, n in seq:
        out.append((op, parts(n, k, stride, k, every, per_step)))
        k += n
    return out


# The driver's op letters: s plain steps, e a held field, p per-step fields, a per-step actions (tests/schedule_alt_driver.cpp).
# b. step(ext, 5), step_actions_traj(7 actions), step_history(None, 4), step_ext_traj(6) under a recorder
RECORDER_CALLS = [("e", 5), ("a", 7), ("s", 4), ("p", 6)]
RECORDER_STRIDE, RECORDER_STRIDE_SINGLE = 3, 1
# c, d. one call of TAPE_T steps on a fresh tape
TAPE_T = 7
TAPE_EVERY = (0, 1, 3, 4, 7)                 # c: pic_tape_start's checkpoint_every
TANGENT_EVERY = (3, 7)                       # d
TAPE_DRIVES = {"actions": "a", "ext_traj": "p", "held": "e"}
# e. T = 5 in single-step parts: a KL or a moments trace cuts every step; tape_step_policy and step_actor step one at a time
SINGLE_T = 5
# f. recorder stride, checkpoint_every, one 7-step step_actions_traj.  (2, 3) cuts at 2, 3, 4 and 6: no part reaches three steps,
# so that case runs the read-only sweep C alone; (3, 4) cuts at 3, 4 and 6 and opens with a part of three.
BOTH_CASES = [(2, 3), (3, 4)]
BOTH_ALTERNATE = {(2, 3): False, (3, 4): True}
# g. an alternating call of 4, then the cached deposit goes, then the call under test (a call of 4 between the two)
FIRST_STEP_CALLS = [("s", 4), ("e", 5), ("s", 4), ("a", 6)]


def test_parts_table():
    """The cut rule on a hand-written table."""
    assert parts(7) == [7]
    assert parts(0) == []
    # a recorder alone: a part ends on every stride-th step counted from start_recording
    assert parts(5, 0, 3) == [3, 2]
    assert parts(7, 5, 3) == [1, 3, 3]
    assert parts(4, 12, 3) == [3, 1]
    assert parts(6, 16, 3) == [2, 3, 1]
    assert parts(4, 0, 1) == [1, 1, 1, 1]
    assert parts(3, 2, 5) == [3]
    # a tape alone: a part ends on every checkpoint step
    assert parts(7, every=3) == [3, 3, 1]
    assert parts(7, every=4) == [4, 3]
    assert parts(7, every=7) == [7]
    assert parts(7, every=1) == [1] * 7
    assert parts(5, tape_steps=2, every=4) == [2, 3]
    # a KL or a moments trace: single steps, whatever the interval
    assert parts(5, every=3, per_step=True) == [1] * 5
    assert parts(5, per_step=True) == [5]                  # (no tape: the flag means nothing)
    # both: the nearer cut wins
    assert parts(7, 0, 2, 0, 3) == [2, 1, 1, 2, 1]
    assert parts(7, 0, 3, 0, 4) == [3, 1, 2, 1]
    assert parts(7, 1, 4, 0, 5) == [3, 2, 2]
    assert [resolved_every(7, k) for k in TAPE_EVERY] == [3, 1, 3, 4, 7]
    assert resolved_every(5, 0) == 3 and resolved_every(5, 9) == 5 and resolved_every(1, 0) == 1
    # the recorder's four calls, as the issue of the GPU tests lists them
    assert [p for _, p in call_sequence(RECORDER_CALLS, stride=3)] == [[3, 2], [1, 3, 3], [3, 1], [2, 3, 1]]


def _alternates(ps):
    return max(ps) >= 3


def test_calls_meant_to_alternate_hold_a_part_of_three():
    """Every call of the GPU tests b, c, d and f that is meant to alternate has a part of three steps or more, and no call of
    test e (or of a case that is there for the single-step parts) has one."""
    for _, ps in call_sequence(RECORDER_CALLS, stride=RECORDER_STRIDE):
        assert _alternates(ps), ps
    for _, ps in call_sequence(RECORDER_CALLS, stride=RECORDER_STRIDE_SINGLE):
        assert max(ps) == 1, ps
    for k in TAPE_EVERY + TANGENT_EVERY:
        ps = parts(TAPE_T, every=resolved_every(TAPE_T, k))
        assert _alternates(ps) == (k != 1), (k, ps)       # (checkpoint_every = 1: the read-only C alone)
    assert parts(SINGLE_T, every=resolved_every(SINGLE_T, 0), per_step=True) == [1] * SINGLE_T
    for (stride, k), want in BOTH_ALTERNATE.items():
        assert _alternates(parts(7, 0, stride, 0, resolved_every(7, k))) == want, (stride, k)
    assert any(BOTH_ALTERNATE.values())
    for _, ps in call_sequence(FIRST_STEP_CALLS):
        assert _alternates(ps), ps


def _script(seq, between=()):
    """The driver script of [(op, [parts])] behind a reset on a handle with read-only C and the alternate stores forced on and
    the light inner steps off (a small state); between: {call index: ops in front of that call}."""
    toks = ["0 0 1 1", "r"]
    for i, (op, ps) in enumerate(seq):
        toks += list(dict(between).get(i, ()))
        toks += ["%s%d" % (op, n) for n in ps]
    return " ".join(toks)


def test_driver_places_y_steps_in_the_parts(tmp_path):
    """The part sequences through the schedule itself: a Y step in every part of three steps or more and in no other, at the
    places tests/test_schedule_alt_cpu.py's rules give; the ring's invariants hold throughout."""
    run = _build(tmp_path, "schedule_alt_driver")
    seqs = [call_sequence(RECORDER_CALLS, stride=RECORDER_STRIDE), call_sequence(RECORDER_CALLS, stride=RECORDER_STRIDE_SINGLE)]
    for op in TAPE_DRIVES.values():
        seqs += [call_sequence([(op, TAPE_T)], every=resolved_every(TAPE_T, k)) for k in TAPE_EVERY]
    seqs += [call_sequence([("a", SINGLE_T)], every=resolved_every(SINGLE_T, 0), per_step=True),      # a KL or a moments trace
             [("a", [1])] * SINGLE_T]                                                          # tape_step_policy, step_actor
    seqs += [call_sequence([("a", 7)], stride=s, every=resolved_every(7, k)) for s, k in BOTH_CASES]
    scripts = [_script(s) for s in seqs]
    # g: the cached deposit dropped (i) in front of the calls under test, as in the GPU test; and, as a contrast for the CPU
    # alone, a copy's ring take behind the drop (i c)
    first = call_sequence(FIRST_STEP_CALLS)
    scripts += [_script(first, {1: ["i"], 3: ["i"]}), _script(first, {1: ["i", "c"], 3: ["i", "c"]})]
    seqs += [first, first]
    for script, seq in zip(scripts, seqs):
        lines = run([script]).splitlines()
        assert check(lines) == 1, script
        want = sum(1 for _, ps in seq for n in ps if n >= 3)
        assert check_alt(lines) == want, (script, want)
        # ... and the parts without one are exactly the others: every op of the script is one call of the output
        ops = [o for _, o, _ in calls(lines) if o[0] in "sepa"]
        assert ops == ["%s%d" % (op, n) for op, ps in seq for n in ps], script
    # g: without a cached deposit each of the two calls under test opens with a sweep A (stage 0): the first script, whose count
    # the GPU test reads in the handle's profile for every way of dropping the deposit.  The second script is a contrast that
    # runs on the CPU alone (no GPU case copies a cached row along): with the row a copy took there is no sweep A
    sweeps_a = [sum(int(f[1]) == 0 for _, _, ls in calls(run([s]).splitlines()) for f in ls) for s in scripts[-2:]]
    assert sweeps_a == [2, 0], sweeps_a


@pytest.mark.parametrize("op", sorted(set("sepa")))
def test_a_part_of_two_never_alternates(tmp_path, op):
    """(what makes a part of three the threshold: the driver on parts of 1, 2 and 3)"""
    run = _build(tmp_path, "schedule_alt_driver")
    assert [check_alt(run(["0 0 1 1 r %s%d" % (op, n)]).splitlines()) for n in (1, 2, 3)] == [0, 0, 1]
