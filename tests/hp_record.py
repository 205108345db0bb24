"""The rollout recorder (csrc/pic_record.h) at its edges, without a GPU: the plan of the particle pass mirrored
(csrc/host_blocks.h: record_plan; tests/test_record_edges_cpu.py pins the mirror against the C++), data that sit on the bin edges
and one storage-ulp beside them, the exact references (NumPy's histograms on the float64 image of what the device holds; entropy,
KL, spectrum rows and field energy in np.longdouble), the derived bounds, a float64 restatement of the finishing sums in the
kernel's order, and the table of cases that tests/test_gpu_record_edges.py runs.  TEST INFRASTRUCTURE ONLY.

Phase-space counts are no part of a record: the finishing kernel turns them into entropy and KL and clears them.  Entropy within
its bound pins the multiset of counts (one count off moves it by about 1/N of a term, the bound is 1e-15 of the terms' sum), and a
KL against a target with a different non-zero value in every bin pins where each count sits (test_record_edges_cpu.py checks
that a single moved particle is seen)."""
import collections

import numpy as np

import hp_reference as hp

LD = hp.LD
U64 = 2.0 ** -53
BLOCK = 512                      # csrc/pic_limits.h
LDS_BYTES = 64 << 10             # csrc/host_blocks.h: kRecordLdsBytes
MARGINAL_BYTES = 32 << 10        # ... and the share of it that the copies of the marginal bins may take
# format name -> (dtype, position_dtype, particles per 16-byte tile)
FORMATS = {"f64": ("float64", None, 2), "f32": ("float32", None, 4), "u32": ("float32", "fixed32", 4)}


# ---- the plan of the particle pass, mirrored ----------------------------------------------------------------------------------------
def plan(N, vec, E, xb, vb, px, pv):
    """{"cols", "gx", "tiles_per_wg", "rr", "phase_lds", "lds"} of record_hist_kernel on E environments of N particles in tiles
    of `vec`: cols tile columns (one tile per lane of a workgroup) per environment, gx workgroups of tiles_per_wg columns each,
    rr LDS copies of every marginal bin, the phase histogram in LDS or not, the dynamic LDS request in bytes."""
    cols = -(-(-(-N // vec)) // BLOCK)
    gx = max(1, min(cols, -(-1024 // E)))
    tpw = -(-cols // gx)
    gx = -(-cols // tpw)
    rr = 16
    while rr > 1 and rr * (xb + vb) * 4 > MARGINAL_BYTES:
        rr //= 2
    marg, prow = (rr * (xb + vb) + 1) * 4, px * (pv + 1) * 4
    phase_lds = int(marg + prow <= LDS_BYTES)
    return {"cols": cols, "gx": gx, "tiles_per_wg": tpw, "rr": rr, "phase_lds": phase_lds, "lds": marg + (prow if phase_lds else 0)}


# ---- data on the edges ---------------------------------------------------------------------------------------------------------------
def around(values, dtype):
    """The images of `values` in `dtype` and the numbers one ulp of `dtype` to either side of each."""
    dtype = np.dtype(dtype).type
    e = np.asarray(values, dtype=np.float64).astype(dtype)
    return np.concatenate([e, np.nextafter(e, dtype(-np.inf)), np.nextafter(e, dtype(np.inf))])


def edge_sets(L, xb, vb, px, pv, vmin, vmax):
    """The float64 edges NumPy bins with: ([position edge sets], [velocity edge sets]); a histogram without bins has none."""
    return ([np.linspace(0, L, nb + 1) for nb in (xb, px) if nb], [np.linspace(vmin, vmax, nb + 1) for nb in (vb, pv) if nb])


def _fill(rng, must, rest, N):
    """N values: all of `must` (a random choice of them if N is smaller), the rest from `rest` in random order, cyclically."""
    if N <= len(must):
        return rng.permutation(must)[:N]
    out = np.concatenate([must, np.resize(rng.permutation(rest), N - len(must))])
    return rng.permutation(out)


def edge_data(dtype, L, xb, vb, px, pv, vmin, vmax, N, seed, nonfinite=False):
    """(x [N], v [N]) in the storage dtype.  Positions: every edge of both position edge sets and one storage-ulp to either side
    (0 and L always: the bounds of `inside`), the rest uniform in [0, L).  Velocities: the same on both velocity edge sets, vmin and
    vmax and one ulp outside each, +-0.0, the rest uniform on a window half as wide again as [vmin, vmax]; with `nonfinite` also
    nan, +inf, -inf.  More edge values than N: a random choice of them.  The two arrays are shuffled independently."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    xe, ve = edge_sets(L, xb, vb, px, pv, vmin, vmax)
    nfill = max(64, N // 4)
    w = vmax - vmin
    x_must = around([0.0, L], dtype)
    x_rest = np.concatenate([around(e, dtype) for e in xe] + [rng.uniform(0, L, nfill).astype(dtype)])
    v_must = np.concatenate([around([vmin, vmax], dtype), np.array([0.0, -0.0], dtype=dtype)]
                            + ([np.array([np.nan, np.inf, -np.inf], dtype=dtype)] if nonfinite else []))
    v_rest = np.concatenate([around(e, dtype) for e in ve] + [rng.uniform(vmin - 0.25 * w, vmax + 0.25 * w, nfill).astype(dtype)])
    x, v = _fill(rng, x_must, x_rest, N), _fill(rng, v_must, v_rest, N)
    assert x.dtype == dtype and v.dtype == dtype and x.shape == v.shape == (N,) and np.isfinite(x).all()
    return x, v


def permuted_pair(x, v, seed):
    """[2, N] arrays: environment 1 holds environment 0's particles in another order."""
    p = np.random.default_rng(seed).permutation(len(x))
    return np.stack([x, x[p]]), np.stack([v, v[p]])


# ---- exact references ------------------------------------------------------------------------------------------------------------------
def counts(x, v, L, xb, vb, px, pv, vmin, vmax):
    """NumPy's histograms of one environment's particles (float64 images of what the device holds): {"x_hist" [xb], "v_hist" [vb],
    "phase" [px, pv] or None, "inside"}."""
    x, v = np.asarray(x), np.asarray(v)
    assert x.dtype == np.float64 and v.dtype == np.float64
    out = {"x_hist": np.histogram(x, bins=xb, range=(0, L))[0] if xb else np.zeros(0, dtype=np.int64),
           "v_hist": np.histogram(v, bins=vb, range=(vmin, vmax))[0] if vb else np.zeros(0, dtype=np.int64),
           "phase": None, "inside": int(np.sum((x >= 0) & (x <= L) & (v >= vmin) & (v <= vmax)))}
    if px:
        out["phase"] = np.histogram2d(x, v, bins=[px, pv], range=[[0, L], [vmin, vmax]])[0].astype(np.int64)
        assert out["phase"].sum() == out["inside"]
    return out


def phase_steps(L, px, pv, vmin, vmax, phase_dx=0.0, phase_dv=0.0):
    """(pdx, pdv) as pic_record_start takes them: an override where one is given, the bins' widths otherwise (float64)."""
    return (phase_dx if phase_dx > 0 else L / px), (phase_dv if phase_dv > 0 else (vmax - vmin) / pv)


def entropy_kl(phase, n0, pdx, pdv, N, feq=None):
    """From exact counts, in longdouble: f = c n0 / pdx / pdv / N; S = -sum f log f pdx pdv over f > 0 and KL = sum f log(f / (feq
    + 1e-12)) pdx pdv (None without feq), each with its term scale T = sum |term| and F = sum f.
    -> {"S", "T_S", "KL", "T_KL", "F"}."""
    c = np.asarray(phase).astype(LD).ravel()
    f = c * (LD(n0) / LD(pdx) / LD(pdv) / LD(N))
    m = f > 0
    a = LD(pdx) * LD(pdv)
    t = f[m] * np.log(f[m])
    out = {"S": -t.sum() * a, "T_S": np.abs(t).sum(), "F": f.sum(), "KL": None, "T_KL": None}
    if feq is not None:
        k = f[m] * np.log(f[m] / (np.asarray(feq, dtype=np.float64).ravel()[m].astype(LD) + LD(1e-12)))
        out["KL"], out["T_KL"] = k.sum() * a, np.abs(k).sum()
    return out


def sum_bound(nb2, T, F, pdx, pdv):
    """|device - longdouble| of an entropy or a KL.  Each term: one rounding for f (and three in its factor n0 / pdx / pdv / N), one
    for the quotient, one for the product, log to 1 ulp, and an error of u in log's argument moves the term by f u: a few u of
    |term| + f.  The sum: 512 strided partial sums of nb2 / 512 terms each, then a tree of 9 levels.  (nb2 / 512 + 16) u (T + 4 F)."""
    return (nb2 / 512 + 16) * U64 * (float(T) + 4 * float(F)) * pdx * pdv


def rows(E_mesh, M):
    """Spectrum rows 0..M-1 of one mesh row, fft(E) / Ng * 2, in longdouble: (re [M], im [M]); row 0 is twice the mean."""
    E = hp.as_ld(E_mesh).ravel()
    re, im = np.zeros(M, dtype=LD), np.zeros(M, dtype=LD)
    if M > 0:
        re[0] = E.sum() / LD(E.size) * 2
    if M > 1:
        re[1:], im[1:] = hp.modes(E_mesh, M - 1)
    return re, im


def rows_bound(E_mesh):
    """The bound of tests/test_gpu_local_parity.py::test_modes_and_feedback_against_longdouble_dft, restated: a sum of Ng products
    with float64 twiddles (each off by u) over a workgroup, then / Ng * 2."""
    E = np.abs(np.asarray(E_mesh, dtype=np.float64))
    return (E.size / 512 + 20) * U64 * 2 * float(E.sum()) / E.size + U64 * float(E.max())


def field_energy(E_mesh, dx):
    E = hp.as_ld(E_mesh).ravel()
    return (E * E).sum() * LD(dx)


def field_energy_bound(E_mesh, dx):
    E = np.asarray(E_mesh, dtype=np.float64)
    return (E.size / 512 + 16) * U64 * float((E * E).sum()) * dx


# ---- the finishing sums restated in float64, in the kernel's order ---------------------------------------------------------------------
def _block_sum(terms):
    """record_finish_kernel's sum of `terms`: thread t of 512 adds terms t, t + 512, ... in order; a wave adds its 64 lanes as
    wave_incl_scan's lane 63 does (rows of 16 by doubling shifts, then (row 3 + row 2) + (row 1 + row 0)); the 8 waves in order."""
    t = np.zeros(-(-max(len(terms), 1) // BLOCK) * BLOCK)
    t[:len(terms)] = terms
    acc = np.zeros(BLOCK)
    for row in t.reshape(-1, BLOCK):
        acc = acc + row
    w = acc.reshape(8, 4, 16)
    for d in (1, 2, 4, 8):
        s = w.copy()
        s[..., d:] = w[..., d:] + w[..., :-d]
        w = s
    r = w[..., 15]
    waves = (r[:, 3] + r[:, 2]) + (r[:, 1] + r[:, 0])
    total = 0.0
    for x in waves:
        total = total + x
    return total


def finish_restated(phase, n0, pdx, pdv, N, feq=None):
    """(entropy, kl) as record_finish_kernel computes them, in float64 NumPy (kl None without feq)."""
    norm = n0 / pdx / pdv / float(N)
    dxdv = pdx * pdv
    f = np.asarray(phase).ravel().astype(np.float64) * norm
    m = f > 0
    s = np.zeros_like(f)
    s[m] = f[m] * np.log(f[m])
    S = -_block_sum(s) * dxdv
    if feq is None:
        return S, None
    k = np.zeros_like(f)
    k[m] = f[m] * np.log(f[m] / (np.asarray(feq, dtype=np.float64).ravel()[m] + 1e-12))
    return S, _block_sum(k) * dxdv


def target(px, pv, seed, zeros=True):
    """A target density [px, pv] with a different value in every bin; with `zeros` a quarter of its bins are exactly zero (a KL
    cannot tell those bins apart: the device tests also take one without)."""
    rng = np.random.default_rng(seed)
    feq = rng.uniform(0.01, 0.05, (px, pv))
    if zeros:
        feq[rng.random((px, pv)) < 0.25] = 0.0
    return feq


# ---- the cases of tests/test_gpu_record_edges.py ---------------------------------------------------------------------------------------
L = 50.0
VMIN, VMAX = -6.1, 7.3            # no float32 numbers
N_ODD = 1027                      # odd, N % 4 == 3
BINS_A = (37, 53, 7, 5)           # x_bins, v_bins, phase x, phase v
BINS_ONE = (1, 1, 1, 1)

Case = collections.namedtuple("Case", "name fmt E N xb vb px pv claim nonfinite load")


def _case(name, fmt, E, N, bins, claim, nonfinite=False, load="reset"):
    return Case(name, fmt, E, N, *bins, claim, nonfinite, load)


def _edges_cases():
    out = []
    for fmt in FORMATS:
        geometry = {"gx": 2 if fmt == "f64" else 1, "tiles_per_wg": 1}
        for tag, bins in (("37x53+7x5", BINS_A), ("1x1+1x1", BINS_ONE)):
            for load in ("reset", "set"):
                out.append(_case(f"edges-{fmt}-{tag}-{load}", fmt, 2, N_ODD, bins, dict(rr=16, phase_lds=1, **geometry), load=load))
        out.append(_case(f"edges-{fmt}-37x53+7x5-nonfinite", fmt, 2, N_ODD, BINS_A, dict(rr=16, phase_lds=1, **geometry), nonfinite=True))
    return out


# (x_bins, v_bins) -> copies of each bin: 16 up to 512 bins in all, then 8, 4, 2, and 1 from 4097
COPIES = [((256, 256), 16), ((257, 256), 8), ((512, 513), 4), ((1024, 1025), 2), ((2048, 2049), 1), ((4096, 4096), 1), ((0, 4096), 2),
          ((4096, 0), 2), ((0, 0), 16)]


def _copies_cases():
    out = []
    for fmt in ("f64", "f32"):
        for (xb, vb), rr in COPIES:
            out.append(_case(f"copies-{fmt}-{xb}x{vb}", fmt, 2, N_ODD, (xb, vb, 7, 5), dict(rr=rr, phase_lds=1)))
        out.append(_case(f"copies-{fmt}-0x0-nophase", fmt, 2, N_ODD, (0, 0, 0, 0), dict(rr=16, phase_lds=1, lds=4)))
    return out


# (marginal bins each, phase x, phase v) -> the phase histogram in LDS, the dynamic LDS request
PHASE = [(0, 127, 128, 1, 65536), (0, 128, 127, 0, 4), (16, 59, 268, 1, 65536), (16, 59, 269, 0, 2052), (0, 4095, 3, 1, 65524),
         (0, 4096, 3, 0, 4), (0, 3, 4096, 1, 49168), (0, 4096, 16, 0, 4), (0, 16, 4096, 0, 4)]


def _phase_cases():
    return [_case(f"phase-{px}x{pv}-marg{mb}", "f64", 2, N_ODD, (mb, mb, px, pv), dict(phase_lds=pl, lds=lds, rr=16))
            for mb, px, pv, pl, lds in PHASE]


def _tails_cases():
    out = []
    for fmt, (_, _, vec) in FORMATS.items():
        for N in (1, 2, 3, 5):
            out.append(_case(f"tails-{fmt}-E1-N{N}", fmt, 1, N, BINS_A, dict(cols=1, gx=1, tiles_per_wg=1)))
        col = BLOCK * vec
        for N in (col - 1, col, col + 1):
            g = 2 if N > col else 1
            out.append(_case(f"tails-{fmt}-E1-N{N}", fmt, 1, N, BINS_A, dict(cols=g, gx=g, tiles_per_wg=1)))
    # a short last workgroup: 3 columns in 2 workgroups of 2; one workgroup over 4 columns
    out.append(_case("tails-f64-E512-N2051", "f64", 512, 2051, BINS_A, dict(cols=3, gx=2, tiles_per_wg=2)))
    out.append(_case("tails-f64-E1025-N3073", "f64", 1025, 3073, BINS_A, dict(cols=4, gx=1, tiles_per_wg=4)))
    return out


# several records: (x_bins, v_bins, phase) with an odd u_stride = x_bins + v_bins + 1, then the bins of a second recording
MULTI = {"lds": ((37, 53, 48, 40), (16, 12, 200, 120)), "global": ((37, 53, 200, 120), (50, 60, 16, 12))}


def _multi_cases():
    out = []
    for fmt in FORMATS:
        for tag, (first, second) in MULTI.items():
            pl = int(tag == "lds")
            out.append(_case(f"multi-{fmt}-{tag}", fmt, 2, N_ODD, first, dict(phase_lds=pl, rr=16)))
            out.append(_case(f"multi-{fmt}-{tag}-restart", fmt, 2, N_ODD, second, dict(phase_lds=1 - pl, rr=16)))
    return out


GROUPS = {"edges": _edges_cases(), "copies": _copies_cases(), "phase": _phase_cases(), "tails": _tails_cases(),
          "multi": _multi_cases()}
CASES = {c.name: c for g in GROUPS.values() for c in g}
assert len(CASES) == sum(len(g) for g in GROUPS.values())


def case_plan(c):
    return plan(c.N, FORMATS[c.fmt][2], c.E, c.xb, c.vb, c.px, c.pv)


def case_data(c):
    """The particles a case is loaded with, [E, N] in the storage dtype: two environments are a permutation of each other, larger
    batches tile three distinct rows (environment e holds row e % 3)."""
    dtype = FORMATS[c.fmt][0]
    seed = sum(map(ord, c.name))
    if c.E <= 2:
        x, v = edge_data(dtype, L, c.xb, c.vb, c.px, c.pv, VMIN, VMAX, c.N, seed, c.nonfinite)
        X, V = permuted_pair(x, v, seed + 1)
        return X[:c.E], V[:c.E]
    three = [edge_data(dtype, L, c.xb, c.vb, c.px, c.pv, VMIN, VMAX, c.N, seed + r) for r in range(3)]
    idx = np.arange(c.E) % 3
    return np.stack([a[0] for a in three])[idx], np.stack([a[1] for a in three])[idx]


# the finishing kernel's scalar cases on a 16 x 16 phase histogram: name -> (n0, vmin, vmax, phase_dx, phase_dv, data)
FINISH_BINS = 16
FINISH_SCALARS = {
    "n0-overrides": (2.5, VMIN, VMAX, 0.37, 0.011, "uniform"),
    "empty-window": (1.0, 100.0, 101.0, 0.0, 0.0, "uniform"),
    "one-bin": (1.0, VMIN, VMAX, 0.0, 0.0, "one-bin"),
    # about four particles per bin and pdx pdv = 4.6 / N: f = c / 4.6 lies around 1, where f log f changes sign, and the terms of
    # either sign all but cancel (test_record_edges_cpu.py: S is below a twentieth of their sum)
    "around-one": (1.0, VMIN, VMAX, 4.6 / N_ODD, 1.0, "uniform"),
}


def finish_data(kind, N, seed):
    """[2, N] float64 positions and velocities of a scalar case: uniform over the box and [VMIN, VMAX], or all in one bin."""
    rng = np.random.default_rng(seed)
    if kind == "one-bin":
        sx, sv = L / FINISH_BINS, (VMAX - VMIN) / FINISH_BINS
        x, v = rng.uniform(5.1 * sx, 5.9 * sx, N), VMIN + rng.uniform(9.1 * sv, 9.9 * sv, N)
    else:
        x, v = rng.uniform(0, L, N), rng.uniform(VMIN, VMAX, N)
    return permuted_pair(x, v, seed + 1)


# meshes and spectrum rows of the finishing kernel: Ng 4 is the smallest a handle accepts (csrc/host_plan.h: check_config)
FINISH_MESHES = (4, 17, 250, 2722)


def finish_modes(Ng):
    return sorted({0, 1, 2, Ng // 2 + 1})
