"""The premises of tests/test_gpu_grad_edges.py on the references alone (no GPU): for every case of tests/hp_grad_cases.py

* the floor of the comparison: the hand-written reverse / forward equations (what the kernels implement) against automatic
  differentiation of the restatement, hp_adjoint.hand_vjp / autograd_vjp, hp_tangent.hand_jvp / torch_jvp and
  hp_tape_kl.hand_vjp / autograd_vjp, below 1e-12 (they show at most 3e-14, 3e-14 and 4e-14, worst on the mesh of 2722 nodes);
* a condition, not a measurement: no sub-stage position q_1..q_4 and no x' of any step of the reference lies within 1e-9 cells of
  a node without lying on it, and only case E's placed particles lie on one, at q_1 of step 0.  A last-bit difference between the
  device's position and the reference's then cannot move a particle into another cell, where the almost-everywhere derivative
  jumps.  A draw that violates it gets another `salt`; the threshold stays.

Case H is checked on its five reference environments."""
import numpy as np
import pytest

import hp_adjoint as ha
import hp_grad_cases as gc


@pytest.mark.parametrize("cid", list(gc.CASES))
def test_hand_equations_agree_with_automatic_differentiation(cid):
    f = gc.floors(cid)
    print(f"grad_edges.{cid}.floor: " + "  ".join(f"{k} {v:.2e}" for k, v in f.items()))
    assert set(f) == {"adjoint", "tangent", "tape_kl"} and gc.CASES[cid].floor == f
    for k, v in f.items():
        assert 0.0 < v < gc.FLOOR_BOUND, (cid, k, v)
        assert gc.bound(cid, 0.0, k) == gc.MARGIN * v


@pytest.mark.parametrize("cid", list(gc.CASES))
def test_no_reference_position_is_within_a_rounding_of_a_node(cid):
    c = gc.CASES[cid]
    lowest = 1.0
    for e in c.ref_envs:
        d = gc.node_distances(cid, e)
        free = np.ones(d.shape, dtype=bool)
        if cid == "E" and e == 0:
            # q_1 of step 0 of the particles placed at rest is their x, exactly: the device and the reference floor the same
            # number.  Sixteen lie on a node; particle 16 lies one rounding under node Ng, by construction and not by accident.
            i = gc.inputs(cid)
            q1 = ha._np_forward_step(i["x"][0], i["v"][0], i["ext"][0, 0], c.setup())[0][0]
            assert c.L / c.Ng == 1.0 and np.array_equal(q1[:17], i["x"][0, :17])
            assert np.all(d[0, 0, :16] == 0.0) and np.floor(q1[16]) == c.Ng - 1 and 0.0 < d[0, 0, 16] < 1e-13
            free[0, 0, :17] = False
            assert q1[17] < 0.0                                   # the particle at x = 0 with v = -1 wraps in the first drift
        assert np.all(d[free] > gc.NODE_DISTANCE), (cid, e, float(d[free].min()))
        lowest = min(lowest, float(d[free].min()))
    print(f"grad_edges.{cid}.node_distance: {lowest:.2e}")


def test_case_table_is_the_one_the_matrix_promises():
    """What each case is there to reach, restated from its numbers (so an edit of the table cannot quietly lose an edge)."""
    C = gc.CASES
    assert list(C) == list("ABCDEFGH")
    assert C["A"].N == 1 and C["B"].N < 64 and C["B"].Ng % 2 == 1 and C["B"].Ng < 64
    assert C["C"].N == 256 + 1 and (C["C"].L, C["C"].n0, C["C"].dt) != (50.0, 1.0, 0.1) and C["C"].T % C["C"].every != 0
    assert C["D"].Ng == 2722 and C["D"].Ng > C["D"].N
    assert C["E"].L / C["E"].Ng == 1.0 and C["E"].N == 2048 + 1
    assert C["F"].dt < 2.0 / np.sqrt(C["F"].N / C["F"].L) < 0.1
    assert C["G"].N % 2 == 1 and C["G"].N > 64 * 256 and C["G"].schedules == (3,)
    assert C["H"].E > 256 and C["H"].N > 2048 and C["H"].schedules == (0,)
    for c in C.values():                                          # no case is silently clamped by the CFL rule of the handle
        assert c.dt <= 2.0 / np.sqrt(c.N / c.L), c.id
    envs = C["H"].ref_envs
    assert len(envs) == 5 and envs[0] == 0 and envs[-1] == 299 and len(set(envs)) == 5
    for k in ("x", "v", "ext", "cot", "cx", "cv"):
        a = gc.inputs("H")[k]
        ax = {"ext": 1, "cot": 2}.get(k, 0)
        assert np.array_equal(np.take(a, 0, ax), np.take(a, 299, ax)) and not np.array_equal(np.take(a, 0, ax), np.take(a, 1, ax))
