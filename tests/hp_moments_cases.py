"""The edge matrix of the fluid moments (include/picstep.h: pic_moments*).  TEST INFRASTRUCTURE ONLY.

The case table, the inputs of every case, the velocity profiles, a NumPy restatement of the header's integer contract
(`quantised_moments`, `quantised_jvp`) and the per-node error bounds of the device against the longdouble references
(`bound`, `jvp_bound`): shared by tests/test_moments_edges_cpu.py (the premises, on the references alone) and
tests/test_gpu_moments_edges.py (the device).  Nothing here was written by reading the kernels: the units, the special values
and the order-freedom are the header's; the rounding allowances are those of tests/hp_checks.py.

Inputs of environment e of a case, all from np.random.default_rng([N, Ng, salt, e]) in this order: x = uniform(0, L, N),
v = normal(0, 2, N), tangents d_x, d_v = standard_normal(N), a cotangent standard_normal((3, Ng)); x and v are then rounded to the
particle dtype.  (N, Ng are the case's nominal ones, whatever mesh a format is given in case D.)  An environment's inputs depend
on its index alone, so any environment can be repeated in a handle of its own.  The first particles of every case with
N >= 63 take hp_checks._planted_positions in the particle dtype (one draw per case, the same in every environment).  `salt` is
what changes if a draw ever violates a premise of test_moments_edges_cpu.py.

No case steps its handle: the moments read the stored state, so no dt clamp can interfere.
"""
import functools
from dataclasses import dataclass

import numpy as np

import hp_checks as hc
import hp_moments as hm
import hp_moments_jvp as hj
import hp_reference as hr

LD = hr.LD
U64 = hc.U64
FORMATS = {"float64": dict(dtype="float64"), "float32": dict(dtype="float32"),
           "fixed32": dict(dtype="float32", position_dtype="fixed32")}
SHAPES = ("CIC", "TSC")
MOMENTS_MESH_LIMIT = 2728     # include/picstep.h: three meshes of 64-bit sums in 64 KB of LDS


@dataclass(frozen=True)
class Case:
    id: str
    E: int
    N: int
    Ng: int                   # the float64 handle's mesh, and the one the draws are seeded with
    L: float
    n0: float
    Ng32: int = 0             # the mesh of the 32-bit formats where it differs (case D)
    salt: int = 0

    def mesh(self, fmt):
        return self.Ng32 if (self.Ng32 and fmt != "float64") else self.Ng

    @property
    def ref_envs(self):
        """The environments the references are evaluated on: all of them, or for case F environments 0, E - 1 and three seeded
        others."""
        if self.E <= 8:
            return tuple(range(self.E))
        mid = np.random.default_rng([self.N, self.Ng, self.salt]).choice(np.arange(1, self.E - 1), 3, replace=False)
        return (0,) + tuple(int(e) for e in np.sort(mid)) + (self.E - 1,)


CASES = {c.id: c for c in (
    Case("A", 2, 1, 4, 50.0, 1.0),                      # bitsN = 0, one lane; 4 cells is pic_create's minimum for CIC and TSC
    Case("B", 3, 63, 5, 50.0, 1.0),                     # under a wave; N % 4 = 3; odd mesh
    Case("C", 2, 1026, 33, 7.7, 0.37),                  # L, n0 off default; N % 4 = 2
    Case("D", 1, 1025, 2722, 50.0, 1.0, Ng32=2728),     # LDS full: pic_create takes 2722 cells in float64; the 32-bit formats
                                                        # take more than the moments' own 2728; N % 4 = 1; most nodes empty
    Case("E", 1, 100001, 250, 50.0, 1.0),               # 13 workgroups per environment, ragged last range
    Case("F", 300, 2100, 16, 10.0, 1.0),                # more environments than CUs; one workgroup each
)}
SCALINGS = {"float64": (-400, -37, -1, 1, 37, 400, 480), "float32": (-100, 100), "fixed32": (-100, 100)}
PROFILE_CASES = ("B", "C")    # the cases the velocity profiles are applied to
RAW_WORDS = ((0, 0), (1, 0xFFFFFFFF))     # fixed32: (particle, raw position word) planted behind the reset


def profiles(fmt):
    """The velocity profiles of a format, by name (see `velocities`)."""
    p = [f"scaled:{k}" for k in SCALINGS[fmt]] + ["outlier", "negative", "pow2_max", "pow2_below"]
    return p + ["m2_below", "m2_at"] if fmt == "float64" else p


def _wtype(fmt):
    return np.dtype(FORMATS[fmt]["dtype"]).type


@functools.lru_cache(maxsize=None)
def _draw(cid, e, fmt):
    c = CASES[cid]
    if cid == "F" and e == c.E - 1:
        e = 0                                   # case F: the last environment is given the first one's inputs
    W = _wtype(fmt)
    rng = np.random.default_rng([c.N, c.Ng, c.salt, e])
    x = rng.uniform(0.0, c.L, c.N).astype(W)
    v = rng.normal(0.0, 2.0, c.N).astype(W)
    d_x, d_v = rng.standard_normal(c.N), rng.standard_normal(c.N)
    cot = rng.standard_normal((3, c.Ng))
    if c.N >= 63:
        like = hc.Case(FORMATS[fmt]["dtype"], "fixed32" if fmt == "fixed32" else "float", "CIC", c.N, c.mesh(fmt), c.L)
        pts = hc._planted_positions(like, np.random.default_rng([c.N, c.Ng, c.salt, 1 << 20]))
        m = min(pts.size, c.N)
        x[:m] = pts[:m]
    for a in (x, v, d_x, d_v, cot):
        a.setflags(write=False)
    return x, v, d_x, d_v, cot


def positions(cid, e, fmt):
    """x [N] of environment e in the particle dtype, as given to the reset (planted positions included)."""
    return _draw(cid, e, fmt)[0]


def tangents(cid, e):
    """(d_x, d_v, cot): two tangents [N] and a cotangent [3, Ng] of environment e (float64 handles)."""
    return _draw(cid, e, "float64")[2:]


def velocities(cid, e, fmt, profile="base"):
    """v [N] of environment e in the particle dtype under a profile of the base draw v ~ N(0, 2):
      base          the draw;
      scaled:k      ldexp(v, k), exact in the particle dtype (pinned by test_moments_edges_cpu.py);
      outlier       particle N // 2 at 2^40, the rest unscaled;
      negative      -|v|;
      pow2_max      the draw scaled so that every |v| <= 3.5, then the largest set to exactly 4.0 (sign kept): max |v| = 2^2 has
                    exponent e = 3;  pow2_below: to nextafter(4.0, 0) in the particle dtype instead: e = 2;
      m2_below      (float64) particle N // 2 at nextafter(2^511, 0): the largest max |v| with a finite m2;
      m2_at         (float64) particle N // 2 at exactly 2^511: m2 = +inf."""
    v = _draw(cid, e, fmt)[1]
    W = v.dtype.type
    if profile == "base":
        return v
    if profile.startswith("scaled:"):
        return np.ldexp(v, int(profile.split(":")[1])).astype(W)
    out = v.copy()
    mid = v.size // 2
    if profile == "outlier":
        out[mid] = W(2.0 ** 40)
    elif profile == "negative":
        out = -np.abs(v)
    elif profile in ("pow2_max", "pow2_below"):
        i = int(np.argmax(np.abs(v)))
        out = (v * (W(3.5) / np.abs(v[i]))).astype(W)
        out[i] = np.copysign(W(4.0) if profile == "pow2_max" else np.nextafter(W(4.0), W(0.0)), v[i])
    elif profile == "m2_below":
        out[mid] = np.nextafter(2.0 ** 511, 0.0)
    elif profile == "m2_at":
        out[mid] = 2.0 ** 511
    else:
        raise ValueError(profile)
    return out


def batch(cid, fmt, profile="base", envs=None):
    """(X, V) [len(envs), N] in the particle dtype: the environments `envs` (all by default) of a case under one profile."""
    envs = range(CASES[cid].E) if envs is None else envs
    return (np.stack([positions(cid, e, fmt) for e in envs]), np.stack([velocities(cid, e, fmt, profile) for e in envs]))


def cell_dtype(fmt):
    return None if fmt == "fixed32" else np.dtype(FORMATS[fmt]["dtype"])


def held(x, fmt, L):
    """The stored position the moments are taken at.  Float formats: np.mod(np.mod(x, L), L) in the particle dtype, the
    reference project's own wrap (a tiny negative x ends on 0, not on L - |x|); x as the handle returns it.  fixed32: x is already
    the uint32 word (every word is a position in [0, L))."""
    x = np.asarray(x)
    if fmt == "fixed32":
        assert x.dtype == np.uint32
        return x
    W = _wtype(fmt)
    Lw = W(L)
    assert float(Lw) <= L                       # (else the exact wrap of hp_reference would fold [L, Lw) again)
    return np.mod(np.mod(x.astype(W), Lw), Lw)


def words_of(cid, e):
    """fixed32 on the CPU: the words of the positions given to the reset (hp_reference.fixed_from_length), RAW_WORDS planted.  The
    GPU tests read the words back from the handle instead."""
    c = CASES[cid]
    w = hr.fixed_from_length(positions(cid, e, "fixed32"), c.L)
    if c.N >= 63:
        for i, raw in RAW_WORDS:
            w[i] = raw
    return w


# ---------------------------------------------------------------------------------------------------------------------------------
# the header's integer contract, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def bits_of(N):
    """b with 2^b >= N."""
    return int(N - 1).bit_length()


def exponent_above(m):
    """e with m < 2^e <= 2 m for a finite m > 0 (max |v| = 4.0 gives 3)."""
    return int(np.frexp(np.float64(m))[1])


def unit_state(vmax):
    """'rest' (all zero), 'nan' (a non-finite value), 'inf2' (max |v| >= 2^511: m2 = +inf), or 'ok'."""
    if not np.isfinite(vmax):
        return "nan"
    if vmax == 0:
        return "rest"
    return "inf2" if vmax >= 2.0 ** 511 else "ok"


def _scale64(N, Ng, L, n0):
    return n0 * L / N / (L / Ng)


def _scale_ld(N, Ng, L, n0):
    return LD(n0) * LD(L) / LD(N) / (LD(L) / LD(Ng))


def _finish(acc, unit_exp, scale):
    """int64 sums -> float64: the conversion rounds once, the unit is a power of two, the scale rounds once."""
    return np.ldexp(acc.astype(np.float64), unit_exp) * scale


def quantised_moments(xh, v, Ng, L, n0=1.0, shape="CIC", cell=None):
    """[3, Ng] float64 by include/picstep.h's contract: every term W_j(x_i) v_i^k (exact weights of the held position, in
    longdouble) rounded half to even to an int64 in the units 2^-fg (m0, the forward's: hp_checks._fg), 2^(e + b - 61) (m1) and
    2^(2e + b - 61) (m2), max |v| < 2^e, 2^b >= N; summed in int64; converted to float64, times the unit, times s.  An
    environment at rest: m1 = m2 = +0; a non-finite velocity: NaN in m1 and m2; max |v| >= 2^511: m2 = +inf."""
    xh, v = np.asarray(xh), np.asarray(v)
    N = xh.shape[0]
    jf, d = hr._cells(xh, Ng, L, cell)
    offs, w = hr.shape_weights(d, shape)
    vmax = float(np.max(np.abs(v.astype(np.float64))))
    state = unit_state(vmax)
    b = bits_of(N)
    e = exponent_above(vmax) if state in ("ok", "inf2") else 0
    ue = (-hc._fg(N), e + b - 61, 2 * e + b - 61)
    vl = hr.as_ld(v)
    acc = np.zeros((3, Ng), dtype=np.int64)
    for o, wk in zip(offs, w):
        nodes = np.mod(jf + o, Ng)
        np.add.at(acc[0], nodes, np.rint(np.ldexp(wk, -ue[0])).astype(np.int64))
        if state in ("ok", "inf2"):
            np.add.at(acc[1], nodes, np.rint(np.ldexp(wk * vl, -ue[1])).astype(np.int64))
        if state == "ok":
            np.add.at(acc[2], nodes, np.rint(np.ldexp(wk * vl * vl, -ue[2])).astype(np.int64))
    s = _scale64(N, Ng, L, n0)
    m = np.zeros((3, Ng))
    m[0] = _finish(acc[0], ue[0], s)
    if state == "nan":
        m[1:] = np.nan
    elif state != "rest":
        m[1] = _finish(acc[1], ue[1], s)
        m[2] = _finish(acc[2], ue[2], s) if state == "ok" else np.inf
    return m


def weight_err(fmt, shape, Ng):
    """Error of one device weight against the exact weight of the held position.
    float64: the forward's own weights, hp_checks._weight_err.
    float32: the shape function in double at d = x / dx - jf with x the held float32 (exact in double), dx = fl(L / Ng) off by
      u64 relative and the quotient (<= Ng) rounded once more: |delta d| <= 2 Ng u64, the difference adds u64 |d|; CIC has slope 1
      in d, TSC at most 2; the polynomial adds 3 u64.
    fixed32: d = frac 2^-32 is exact in double; 1 - d resp. the polynomial add up to 3 u64."""
    k = 1 if shape == "CIC" else 2
    if fmt == "float64":
        return hc._weight_err(hc.Case("float64", "float", shape, 1, Ng, 1.0))
    if fmt == "float32":
        return (k * (2 * Ng + 1) + 3) * U64
    return 3 * U64


def node_terms(xh, v, Ng, L, shape="CIC", cell=None):
    """What `bound` needs of one environment, per node j and moment k: count [Ng] (terms deposited on j), absw [3, Ng] =
    sum |W_j(x_i)| |v_i|^k and vsum [3, Ng] = sum |v_i|^k over the particles that touch j (longdouble), and vmax, N."""
    xh, v = np.asarray(xh), np.asarray(v)
    jf, d = hr._cells(xh, Ng, L, cell)
    offs, w = hr.shape_weights(d, shape)
    av = np.abs(hr.as_ld(v))
    pw = (np.ones_like(av), av, av * av)
    count = np.zeros(Ng, dtype=np.int64)
    absw, vsum = np.zeros((3, Ng), dtype=LD), np.zeros((3, Ng), dtype=LD)
    for o, wk in zip(offs, w):
        nodes = np.mod(jf + o, Ng)
        count += np.bincount(nodes, minlength=Ng)
        for k in range(3):
            np.add.at(absw[k], nodes, np.abs(wk) * pw[k])
            np.add.at(vsum[k], nodes, pw[k])
    return dict(count=count, absw=absw, vsum=vsum, vmax=float(np.max(np.abs(v.astype(np.float64)))), N=xh.shape[0])


def bound(c, profile, ref, counts, fmt="float64", shape="CIC"):
    """[3, Ng] longdouble bound on |m_k,j(device) - m_k,j(longdouble)|, from the arithmetic the header states.

    A term of moment k is t = round(fl(fl(w' v) v) / U_k) with w' the device's weight, |w' - w| <= werr (weight_err), and U_k the
    unit: 2^-fg, 2^(e + b - 61), 2^(2e + b - 61).  Against the exact w v^k:
        |t U_k - w v^k|  <=  U_k / 2  +  werr |v|^k  +  (k + 1) u64 (|w| + werr) |v|^k
    (half a unit; the weight's own error; k roundings of the products, one more for second-order terms).  The integer sum is
    exact, so on node j with count_j terms, absw = sum |w| |v|^k and vsum = sum |v|^k over its particles
        D_k,j = s (count_j U_k / 2 + werr vsum_k,j + (k + 1) u64 (absw_k,j + werr vsum_k,j)),
    and the conversion (double)sum, the host's scale n0 L / N / dx (four roundings) and its product add, as in
    hp_checks.density_bound, 6 u64 (|m_k,j| + D_k,j).
    The half unit does not shrink where a node holds slow particles only: with one fast particle in the environment every
    node's m1 / m2 is resolved to N 2^-61 of N max|v|^k, the header's statement, and no finer (profile `outlier`).
    Row 2 is meaningless for profile m2_at (m2 = +inf there); rows 1, 2 for an environment at rest are 0 (+0 exactly)."""
    Ng = c.mesh(fmt)
    N = counts["N"]
    s = _scale_ld(N, Ng, c.L, c.n0)
    werr = LD(weight_err(fmt, shape, Ng))
    state = unit_state(counts["vmax"])
    assert state != "nan" and (state == "ok" or profile == "m2_at" or counts["vmax"] == 0), (profile, state)
    e = exponent_above(counts["vmax"]) if state != "rest" else 0
    b = bits_of(N)
    half = [np.ldexp(LD(1), -hc._fg(N) - 1), np.ldexp(LD(1), e + b - 62), np.ldexp(LD(1), 2 * e + b - 62)]
    out = np.zeros((3, Ng), dtype=LD)
    cnt = counts["count"].astype(LD)
    for k in range(3):
        if k and state == "rest":
            continue
        D = s * (cnt * half[k] + werr * counts["vsum"][k] + (k + 1) * LD(U64) * (counts["absw"][k] + werr * counts["vsum"][k]))
        out[k] = D + 6 * LD(U64) * (np.abs(ref[k]) + D)
    return out


def check_rows(got, ref, bnd, rows=(0, 1, 2)):
    """(worst ratio |got - ref| / bound over the rows' nodes, worst max-normalised error max_j |dm_k| / max_j |m_k|).  Where the
    bound is 0 the device must be exact (ratio 0, or inf)."""
    worst = norm = 0.0
    for k in rows:
        err = np.abs(np.asarray(got[k]).astype(LD) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bnd[k] > 0, err / np.where(bnd[k] > 0, bnd[k], 1), np.where(err == 0, 0, np.inf))
        worst = max(worst, float(np.max(r)))
        den = float(np.max(np.abs(ref[k])))
        if den > 0:
            norm = max(norm, float(np.max(err)) / den)
    return worst, norm


# ---------------------------------------------------------------------------------------------------------------------------------
# the forward mode (float64, CIC)
# ---------------------------------------------------------------------------------------------------------------------------------
def jvp_words(v, d_x, d_v, Ng, L):
    """The three bound words of one (direction, environment) in float64, as the header writes them: with iota = d_x / dx,
    b0 = max |iota|, b1 = max (|d_v| + |iota v|), b2 = max (2 |v d_v| + |iota| v^2).  d_x, d_v: arrays or None (0)."""
    v = np.asarray(v, dtype=np.float64)
    z = np.zeros_like(v)
    dxs = z if d_x is None else np.asarray(d_x, dtype=np.float64)
    dvs = z if d_v is None else np.asarray(d_v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        io = np.abs(dxs / (L / Ng))
        words = (io, np.abs(dvs) + np.abs(io * v), 2.0 * np.abs(v * dvs) + io * (v * v))
        return tuple(float(np.max(w)) if np.isfinite(w).all() else float("inf") for w in words)


def _jvp_parts(xh, v, d_x, d_v, Ng, L):
    """Per particle and moment the two terms (left, right node) in longdouble, their nodes, and the sums of absolute parts."""
    jf, d = hr._cells(xh, Ng, L, np.float64)
    vl = hr.as_ld(v)
    z = np.zeros(vl.shape, dtype=LD)
    dxs = z if d_x is None else hr.as_ld(d_x)
    dvs = z if d_v is None else hr.as_ld(d_v)
    io = dxs / (LD(L) / LD(Ng))
    wl, wr = 1 - d, d
    left = (-io, wl * dvs - io * vl, 2 * wl * vl * dvs - io * vl * vl)
    right = (io, wr * dvs + io * vl, 2 * wr * vl * dvs + io * vl * vl)
    aio = np.abs(io)
    mag_l = (aio, np.abs(wl * dvs) + aio * np.abs(vl), 2 * np.abs(wl * vl * dvs) + aio * vl * vl)
    mag_r = (aio, np.abs(wr * dvs) + aio * np.abs(vl), 2 * np.abs(wr * vl * dvs) + aio * vl * vl)
    dpart = (z, np.abs(dvs), 2 * np.abs(vl * dvs))            # what a weight's error multiplies
    return np.mod(jf, Ng), np.mod(jf + 1, Ng), left, right, mag_l, mag_r, dpart


def quantised_jvp(xh, v, d_x, d_v, Ng, L, n0=1.0):
    """[3, Ng] float64 by the header's contract for pic_moments_jvp: every term of the table an int64 in the unit
    2^(e_m + b - 61), b_m < 2^e_m the moment's bound word; a zero word: +0; a non-finite word: NaN in that moment."""
    N = np.asarray(xh).shape[0]
    jl, jr, left, right, _, _, _ = _jvp_parts(xh, v, d_x, d_v, Ng, L)
    words = jvp_words(v, d_x, d_v, Ng, L)
    s = _scale64(N, Ng, L, n0)
    out = np.zeros((3, Ng))
    for m in range(3):
        if not np.isfinite(words[m]):
            out[m] = np.nan
            continue
        if words[m] == 0:
            continue
        ue = exponent_above(words[m]) + bits_of(N) - 61
        acc = np.zeros(Ng, dtype=np.int64)
        if m == 0:
            r = np.rint(np.ldexp(right[0], -ue)).astype(np.int64)      # both halves are one rounded integer
            np.add.at(acc, jl, -r)
            np.add.at(acc, jr, r)
        else:
            np.add.at(acc, jl, np.rint(np.ldexp(left[m], -ue)).astype(np.int64))
            np.add.at(acc, jr, np.rint(np.ldexp(right[m], -ue)).astype(np.int64))
        out[m] = _finish(acc, ue, s)
    return out


def jvp_ld(xh, v, d_x, d_v, Ng, L, n0=1.0):
    """hp_moments_jvp.jvp_ld at the held positions (the forward's float64 cell)."""
    return hj.jvp_ld(xh, v, d_x, d_v, Ng, L, n0, np.float64)


def jvp_bound(c, ref, xh, v, d_x, d_v):
    """[3, Ng] longdouble bound on |dm(device) - dm(longdouble)| for one (direction, environment), float64 + CIC.

    A term of moment m is round(fl(term) / U_m), U_m = 2^(e_m + b - 61) from the moment's bound word b_m < 2^e_m.  fl(term)
    evaluates w' d_v -/+ iota v (resp. 2 w' v d_v -/+ iota v^2, resp. iota) in float64: iota = d_x / dx carries dx's rounding
    and the division's (2 u64), every product and the sum one more each, at most 4 u64 of the sum of the absolute parts
    (mag); the weight's own error (hp_checks._weight_err) multiplies |d_v| resp. 2 |v d_v| (dpart).  On node j:
        D_m,j = s (count_j U_m / 2 + werr sum dpart + 4 u64 sum mag),
    plus 6 u64 (|dm_m,j| + D_m,j) for the conversion, the scale and its product (as `bound`).  A zero word: the row is +0 and
    its bound 0."""
    Ng, N = c.Ng, np.asarray(xh).shape[0]
    jl, jr, _, _, mag_l, mag_r, dpart = _jvp_parts(xh, v, d_x, d_v, Ng, c.L)
    words = jvp_words(v, d_x, d_v, Ng, c.L)
    s = _scale_ld(N, Ng, c.L, c.n0)
    werr = LD(weight_err("float64", "CIC", Ng))
    cnt = (np.bincount(jl, minlength=Ng) + np.bincount(jr, minlength=Ng)).astype(LD)
    out = np.zeros((3, Ng), dtype=LD)
    for m in range(3):
        assert np.isfinite(words[m])
        if words[m] == 0:
            continue
        half = np.ldexp(LD(1), exponent_above(words[m]) + bits_of(N) - 62)
        mag, dp = np.zeros(Ng, dtype=LD), np.zeros(Ng, dtype=LD)
        for nodes, mg in ((jl, mag_l[m]), (jr, mag_r[m])):
            np.add.at(mag, nodes, mg)
            np.add.at(dp, nodes, dpart[m])
        D = s * (cnt * half + werr * dp + 4 * LD(U64) * mag)
        out[m] = D + 6 * LD(U64) * (np.abs(ref[m]) + D)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the gather (float64, CIC)
# ---------------------------------------------------------------------------------------------------------------------------------
def vjp_ld(xh, v, g, Ng, L, n0=1.0):
    """hp_moments.hand_vjp's equations in longdouble at the held positions (the forward's float64 cell, exact weights)."""
    N = np.asarray(xh).shape[0]
    jf, d = hr._cells(xh, Ng, L, np.float64)
    jl, jr = np.mod(jf, Ng), np.mod(jf + 1, Ng)
    vl, g = hr.as_ld(v), hr.as_ld(g)
    dx = LD(L) / LD(Ng)
    s = _scale_ld(N, Ng, L, n0)
    slope = lambda a: (a[jr] - a[jl]) / dx  # noqa: E731
    gx = s * (slope(g[0]) + vl * slope(g[1]) + vl * vl * slope(g[2]))
    gv = s * (((1 - d) * g[1][jl] + d * g[1][jr]) + 2 * vl * ((1 - d) * g[2][jl] + d * g[2][jr]))
    return gx, gv


VJP_BOUND = 1.7e-14           # tests/test_gpu_moments.py: VJP_BOUND (relative norm)
VJP_CEILING = 1e-9            # hp_grad_cases.CEILING
VJP_CASES = ("A", "B", "C")


@functools.lru_cache(maxsize=None)
def vjp_floor(cid):
    """The hand equations against autograd (float64 both) at the case, in the relative norm, worst over the environments."""
    import hp_adjoint as ha
    c = CASES[cid]
    S = ha.Setup(c.N, c.Ng, c.L, c.n0, 0.1)
    worst = 0.0
    for e in c.ref_envs:
        x, v, g = (np.array(a) for a in (positions(cid, e, "float64"), velocities(cid, e, "float64"), tangents(cid, e)[2]))
        for a, b in zip(hm.hand_vjp(x, v, g, S), hm.autograd_vjp(x, v, g, S)):
            worst = max(worst, float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)))
    return worst


def vjp_bound(cid):
    """max(test_gpu_moments.py's VJP_BOUND, 100 x the case's floor): grad-edges' rule, never above its ceiling."""
    b = max(VJP_BOUND, 100.0 * vjp_floor(cid))
    assert b <= VJP_CEILING, (cid, b)
    return b
