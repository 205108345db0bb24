"""The premises of tests/test_gpu_record_edges.py, without a GPU: the plan of the recorder's particle pass (csrc/host_blocks.h:
record_plan) through a stand-alone driver against a hand-written table and the mirror hp_record.plan, the plan values every device
case is named for, the bound of the finishing sums against a float64 restatement in the kernel's order, and the edge data."""
import itertools
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import hp_record as hr
from conftest import record_measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimal-control-1d-electrostatic-plasma_amd", "csrc")


# ---- 1. the planner ------------------------------------------------------------------------------------------------------------------
def _build(tmp, name, extra):
    out = str(tmp / name)
    args = ["-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + extra + [os.path.join(ROOT, "tests", "record_plan_driver.cpp"), "-o", out]
    cxx = shutil.which("c++")
    if cxx:
        cmd = [cxx] + args
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no host C++ compiler (c++ or hipcc) to build tests/record_plan_driver.cpp with")
        cmd = [hipcc, "-x", "c++"] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        p = subprocess.run([out], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        res = p.stdout.splitlines()
        assert len(res) == len(lines)
        return res
    return run


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_plan")
    return (_build(tmp, "record_plan_driver", []),
            _build(tmp, "record_plan_driver_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


PLAN_TABLE = [
    # N, vec, E, xb, vb, px, pv -> gx, tiles_per_wg, rr, phase_lds, lds
    ((20000, 2, 3, 37, 53, 48, 40), (20, 1, 16, 1, 13636)),          # tests/test_gpu_record.py: 5764 B of marginals + 48 rows of 41 words
    ((20000, 2, 3, 37, 53, 200, 120), (20, 1, 16, 0, 5764)),         # ... and 96800 B of phase rows: global atomics
    ((1000000, 2, 64, 64, 64, 64, 64), (16, 62, 16, 1, 24836)),      # its workload: 977 columns in 16 workgroups of 62 (the last: 47)
    ((5000, 4, 256, 64, 64, 64, 64), (3, 1, 16, 1, 24836)),
    ((1027, 2, 2, 0, 0, 127, 128), (2, 1, 16, 1, 65536)),            # 4 + 127 * 129 * 4: the whole of the LDS
    ((1027, 2, 2, 0, 0, 128, 127), (2, 1, 16, 0, 4)),                # 4 + 128 * 128 * 4: four bytes too many
    ((1027, 2, 2, 16, 16, 59, 268), (2, 1, 16, 1, 65536)),           # 2052 + 59 * 269 * 4
    ((1027, 2, 2, 16, 16, 59, 269), (2, 1, 16, 0, 2052)),
    ((2051, 2, 512, 37, 53, 7, 5), (2, 2, 16, 1, 5932)),             # 3 columns: the second workgroup has one
    ((3073, 2, 1025, 37, 53, 7, 5), (1, 4, 16, 1, 5932)),            # more environments than workgroups wanted: one each
    ((1027, 4, 2, 256, 256, 7, 5), (1, 1, 16, 1, 32940)),            # 512 bins: 16 copies are 32 KiB
    ((1027, 4, 2, 257, 256, 7, 5), (1, 1, 8, 1, 16588)),
    ((1027, 4, 2, 4096, 0, 7, 5), (1, 1, 2, 1, 32940)),
    ((1027, 4, 2, 4096, 4096, 7, 5), (1, 1, 1, 1, 32940)),
    ((1, 2, 1, 0, 0, 0, 0), (1, 1, 16, 1, 4)),                       # the word of `inside` alone
    ((1 << 36, 2, 1, 0, 0, 0, 0), (1024, 65536, 16, 1, 4)),          # the largest N a handle accepts
]


def _line(N, vec, E, xb, vb, px, pv):
    return f"plan {N} {vec} {E} {xb} {vb} {px} {pv}"


def _fmt(p):
    return f"ok gx={p['gx']} tiles_per_wg={p['tiles_per_wg']} rr={p['rr']} phase_lds={p['phase_lds']} lds={p['lds']}"


def test_record_plan_table_and_mirror(drivers):
    for args, (gx, tpw, rr, pl, lds) in PLAN_TABLE:
        p = hr.plan(*args)
        assert (p["gx"], p["tiles_per_wg"], p["rr"], p["phase_lds"], p["lds"]) == (gx, tpw, rr, pl, lds), args
    bins = sorted({(c.xb, c.vb, c.px, c.pv) for c in hr.CASES.values()} | {(64, 64, 64, 64), (4096, 4096, 4096, 4096)})
    assert len(bins) > 25
    shapes = [a for a, _ in PLAN_TABLE]
    shapes += [(N, vec, E) + b for E, N, vec, b in itertools.product(
        (1, 2, 3, 512, 1024, 1025, 4096), (1, 2, 3, 5, 1023, 1024, 1025, 2047, 2048, 2049, 2051, 3073, 10 ** 6), (2, 4), bins)]
    lines = [_line(*s) for s in shapes]
    for run in drivers:
        for s, got in zip(shapes, run(lines)):
            assert got == _fmt(hr.plan(*s)), s
    for N, vec, E, xb, vb, px, pv in shapes:
        p = hr.plan(N, vec, E, xb, vb, px, pv)
        # the workgroups cover every column, and none of them is empty
        assert p["gx"] * p["tiles_per_wg"] >= p["cols"] > (p["gx"] - 1) * p["tiles_per_wg"], (N, vec, E)
        assert p["cols"] * hr.BLOCK * vec >= N > (p["cols"] - 1) * hr.BLOCK * vec
        # the most copies that fit 32 KiB, a power of two, at least one
        rr = p["rr"]
        assert rr in (1, 2, 4, 8, 16) and (rr == 1 or rr * (xb + vb) * 4 <= hr.MARGINAL_BYTES), (xb, vb)
        assert rr == 16 or 2 * rr * (xb + vb) * 4 > hr.MARGINAL_BYTES, (xb, vb)
        # the phase histogram is in LDS exactly when everything fits 64 KiB, and the request is what the kernel lays out
        marg, prow = (rr * (xb + vb) + 1) * 4, px * (pv + 1) * 4
        assert p["phase_lds"] == int(marg + prow <= hr.LDS_BYTES) and p["lds"] == marg + p["phase_lds"] * prow <= hr.LDS_BYTES


def test_pic_record_start_has_no_layout_arithmetic_of_its_own():
    src = open(os.path.join(CSRC, "picstep.hip")).read()
    body = src[src.index("int pic_record_start("):src.index("int pic_record_now(")]
    assert "record_plan(" in body
    for word in ("rr /=", "<< 10", "tiles_per_wg =", "BLOCK", "sizeof(unsigned) >"):
        assert word not in body, word


# ---- 2. every device case runs the path it is named for ---------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(hr.GROUPS))
def test_cases_are_on_their_claimed_paths(group):
    for c in hr.GROUPS[group]:
        p = hr.case_plan(c)
        assert c.claim and {k: p[k] for k in c.claim} == c.claim, (c.name, p)
        assert p["lds"] <= hr.LDS_BYTES


def test_case_table_covers_what_it_is_for():
    plans = {n: hr.case_plan(c) for n, c in hr.CASES.items()}
    assert {plans[c.name]["rr"] for c in hr.GROUPS["copies"]} == {1, 2, 4, 8, 16}
    # both sides of both thresholds, one byte-exact
    ph = hr.GROUPS["phase"]
    assert sum(plans[c.name]["lds"] == hr.LDS_BYTES for c in ph) == 2 and {plans[c.name]["phase_lds"] for c in ph} == {0, 1}
    # the particle tail: every residue of N modulo the tile, one and several workgroups, a short last workgroup, several columns in one
    for fmt, (_, _, vec) in hr.FORMATS.items():
        assert {c.N % vec for c in hr.GROUPS["tails"] if c.fmt == fmt} == set(range(vec))
    t = [plans[c.name] for c in hr.GROUPS["tails"]]
    assert any(p["gx"] > 1 and p["gx"] * p["tiles_per_wg"] > p["cols"] for p in t) and any(p["gx"] == 1 and p["tiles_per_wg"] > 1 for p in t)
    for c in hr.CASES.values():
        if c.name.startswith("multi") and not c.name.endswith("restart"):
            assert (c.xb + c.vb + 1) % 2 == 1                     # an odd u_stride
    assert hr.N_ODD % 4 == 3 and all(np.float64(np.float32(b)) != b for b in (hr.VMIN, hr.VMAX))


# ---- 3. the bound of the finishing sums is the device's to miss ---------------------------------------------------------------------------
def _phase_inputs():
    """(name, phase counts, n0, pdx, pdv, N, feq) of every entropy / KL a device test holds against hp_record.sum_bound."""
    for group in ("edges", "copies", "phase", "tails", "multi"):
        for c in hr.GROUPS[group]:
            if not c.px or c.nonfinite or c.E > 2:
                continue
            X, V = hr.case_data(c)
            ph = hr.counts(X[0].astype(np.float64), V[0].astype(np.float64), hr.L, c.xb, c.vb, c.px, c.pv, hr.VMIN, hr.VMAX)["phase"]
            pdx, pdv = hr.phase_steps(hr.L, c.px, c.pv, hr.VMIN, hr.VMAX)
            yield c.name, ph, 1.0, pdx, pdv, c.N, hr.target(c.px, c.pv, 5)
            if group == "phase":
                yield c.name + "-dense", ph, 1.0, pdx, pdv, c.N, hr.target(c.px, c.pv, 6, zeros=False)
    nb = hr.FINISH_BINS
    for name, (n0, vmin, vmax, pdx, pdv, kind) in hr.FINISH_SCALARS.items():
        X, V = hr.finish_data(kind, hr.N_ODD, 7)
        ph = hr.counts(X[0], V[0], hr.L, 0, 0, nb, nb, vmin, vmax)["phase"]
        yield name, ph, n0, *hr.phase_steps(hr.L, nb, nb, vmin, vmax, pdx, pdv), hr.N_ODD, hr.target(nb, nb, 5)


def test_restated_finishing_sums_are_inside_the_bound():
    worst = {"entropy": 0.0, "kl": 0.0}
    n = 0
    for name, ph, n0, pdx, pdv, N, feq in _phase_inputs():
        r = hr.entropy_kl(ph, n0, pdx, pdv, N, feq)
        S, K = hr.finish_restated(ph, n0, pdx, pdv, N, feq)
        for key, got, want, T in (("entropy", S, r["S"], r["T_S"]), ("kl", K, r["KL"], r["T_KL"])):
            b = hr.sum_bound(ph.size, T, r["F"], pdx, pdv)
            err = float(abs(hr.LD(got) - want))
            assert err <= b, (name, key, err, b)
            if b > 0:
                worst[key] = max(worst[key], err / b)
        n += 1
    assert n > 60 and 0 < worst["entropy"] < 1 and 0 < worst["kl"] < 1, worst
    record_measure("record_edges.restatement.entropy", worst["entropy"])
    record_measure("record_edges.restatement.kl", worst["kl"])


def test_scalar_cases_are_what_they_are_named_for():
    nb = hr.FINISH_BINS
    ref = {}
    for name, (n0, vmin, vmax, pdx, pdv, kind) in hr.FINISH_SCALARS.items():
        X, V = hr.finish_data(kind, hr.N_ODD, 7)
        ph = hr.counts(X[0], V[0], hr.L, 0, 0, nb, nb, vmin, vmax)["phase"]
        ref[name] = (ph, hr.entropy_kl(ph, n0, *hr.phase_steps(hr.L, nb, nb, vmin, vmax, pdx, pdv), hr.N_ODD))
    assert ref["empty-window"][0].sum() == 0 and ref["empty-window"][1]["S"] == 0
    assert np.count_nonzero(ref["one-bin"][0]) == 1 and ref["one-bin"][0].max() == hr.N_ODD
    ph, r = ref["around-one"]
    f = ph / 4.6
    assert (f < 1).sum() > 64 and (f > 1).sum() > 64
    pdx, pdv = hr.FINISH_SCALARS["around-one"][3:5]
    # S cancels to a small part of its terms' sum: a bound relative to S would be the wrong scale here
    assert abs(float(r["S"])) < 0.05 * float(r["T_S"]) * pdx * pdv


def test_kl_sees_a_single_moved_particle():
    """Phase counts are no part of a record: a KL within its bound is the check of where each count sits.  Moving one particle
    to another bin moves the KL against a target without zero bins by far more than twice the bound, whichever bins are taken
    (between two zero bins of a target the move may not show at all: the device tests take both targets)."""
    rng = np.random.default_rng(1)
    for c in hr.GROUPS["phase"]:
        X, V = hr.case_data(c)
        ph = hr.counts(X[0].astype(np.float64), V[0].astype(np.float64), hr.L, c.xb, c.vb, c.px, c.pv, hr.VMIN, hr.VMAX)["phase"]
        pdx, pdv = hr.phase_steps(hr.L, c.px, c.pv, hr.VMIN, hr.VMAX)
        feq = hr.target(c.px, c.pv, 6, zeros=False)
        r = hr.entropy_kl(ph, 1.0, pdx, pdv, c.N, feq)
        b = hr.sum_bound(ph.size, r["T_KL"], r["F"], pdx, pdv)
        full = np.flatnonzero(ph.ravel())
        for _ in range(20):
            i, j = rng.choice(full), rng.integers(ph.size)
            if i == j:
                continue
            moved = ph.ravel().copy()
            moved[i] -= 1
            moved[j] += 1
            r2 = hr.entropy_kl(moved, 1.0, pdx, pdv, c.N, feq)
            b2 = hr.sum_bound(ph.size, r2["T_KL"], r2["F"], pdx, pdv)
            assert abs(float(r2["KL"] - r["KL"])) > 1e6 * (b + b2), (c.name, i, j)


# ---- 4. the edge data --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edge_data_holds_the_edges_and_their_neighbours(dtype):
    xb, vb, px, pv = hr.BINS_A
    x, v = hr.edge_data(dtype, hr.L, xb, vb, px, pv, hr.VMIN, hr.VMAX, hr.N_ODD, 3)
    xe, ve = hr.edge_sets(hr.L, xb, vb, px, pv, hr.VMIN, hr.VMAX)
    for vals, sets in ((x, xe), (v, ve)):
        have = np.unique(vals)
        have64 = have.astype(np.float64)
        for edges in sets:
            for e in edges:
                i = np.searchsorted(have64, e, side="right") - 1
                below = have[i]
                assert below <= e
                if have64[i] == e:            # on the edge, with the numbers one ulp below and above it
                    assert have[i - 1] == np.nextafter(below, dtype(-np.inf)) and have[i + 1] == np.nextafter(below, dtype(np.inf)), e
                else:                         # no number of the dtype is on this edge: the two that enclose it
                    assert dtype is np.float32 and have[i + 1] == np.nextafter(below, dtype(np.inf)) and have64[i + 1] > e, e
            if dtype is np.float64:           # every float64 edge is held exactly, and NumPy puts its lower neighbour a bin lower
                assert np.isin(edges, have).all()
                inner = edges[1:-1]
                bins = np.searchsorted(edges, inner, side="right") - 1
                assert np.array_equal(np.searchsorted(edges, np.nextafter(inner, -np.inf), side="right") - 1, bins - 1)
    # the window's ends, one ulp outside each, both zeros, values well outside, no non-finite value unless asked for
    lo, hi = dtype(hr.VMIN), dtype(hr.VMAX)
    for special in (lo, hi, np.nextafter(lo, dtype(-np.inf)), np.nextafter(hi, dtype(np.inf))):
        assert (v == special).any()
    assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
    assert (v < hr.VMIN - 1).any() and (v > hr.VMAX + 1).any() and np.isfinite(v).all()
    assert (x == 0).any() and (x == dtype(hr.L)).any() and (x < 0).any() and (x > hr.L).any()
    assert not np.array_equal(np.argsort(x, kind="stable"), np.argsort(v, kind="stable"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_numpy_drops_non_finite_velocities_without_a_warning(dtype):
    xb, vb, px, pv = hr.BINS_A
    x, v = hr.edge_data(dtype, hr.L, xb, vb, px, pv, hr.VMIN, hr.VMAX, hr.N_ODD, 3, nonfinite=True)
    assert np.isnan(v).sum() == 1 and (v == np.inf).sum() == 1 and (v == -np.inf).sum() == 1 and np.isfinite(x).all()
    x64, v64 = x.astype(np.float64), v.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c = hr.counts(x64, v64, hr.L, xb, vb, px, pv, hr.VMIN, hr.VMAX)
    ok = np.isfinite(v64)
    d = hr.counts(x64[ok], v64[ok], hr.L, xb, vb, px, pv, hr.VMIN, hr.VMAX)
    assert np.array_equal(c["v_hist"], d["v_hist"]) and np.array_equal(c["phase"], d["phase"]) and c["inside"] == d["inside"]
    assert c["x_hist"].sum() == d["x_hist"].sum() + np.sum((x64[~ok] >= 0) & (x64[~ok] <= hr.L))       # x_hist does not look at v


def test_edge_data_fits_any_size():
    for N in (1, 2, 3, 5, 2049):
        for bins in (hr.BINS_A, hr.BINS_ONE, (4096, 4096, 4096, 16), (0, 0, 0, 0)):
            x, v = hr.edge_data(np.float32, hr.L, *bins, hr.VMIN, hr.VMAX, N, 9, nonfinite=N >= 16)
            assert x.shape == v.shape == (N,)
    X, V = hr.case_data(hr.CASES["tails-f64-E1025-N3073"])
    assert X.shape == V.shape == (1025, 3073) and np.array_equal(X[3], X[0]) and not np.array_equal(X[1], X[0])
    X, V = hr.case_data(hr.CASES["edges-f32-37x53+7x5-reset"])
    assert X.dtype == np.float32 and not np.array_equal(X[0], X[1]) and np.array_equal(np.sort(X[0]), np.sort(X[1]))
    assert np.array_equal(np.sort(V[0]), np.sort(V[1]))
