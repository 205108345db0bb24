"""The edge cases of the smoothed phase-space density, its KL, the gradient gather and the forward-mode product (DESIGN.md 7g,
7j).  TEST INFRASTRUCTURE ONLY.

The case table, the deterministic edge state of every case and a np.longdouble reference of the hand equations, evaluated once
per process: shared by tests/test_phase_edges_cpu.py (the premises, on the references alone) and tests/test_gpu_phase_edges.py
(the device).  The reference uses no automatic differentiation, so a NaN particle cannot spread: the density comes from
hp_phase.density (exact integer sums, then the device's two float64 products), everything behind it is longdouble arithmetic on
hp_phase.locate's bins and fractions.

Environment 0's first particles are the cross product of `positions` and `velocities`, in anti-diagonal order (pair (i, j) before
(i', j') if i + j < i' + j', then by i) and truncated at N, so that a small N still meets the head of both lists; the rest are
uniform in [0, L) and in the v range widened by 20 % on both sides, from default_rng([N, nx, nv]).

A state reaches the handle in one of two ways (LOADS), and the kernels see different particles after each.  "reset": pic_reset's
refresh stores the wrapped positions ("the stored, wrapped x"), so x = L, -0.0 and a tiny negative x become 0,
nextafter(L, 2L) becomes one ulp of L, and a NaN or inf position is parked at 0 -- inside the box if its v is; v stays as given.
No particle is dropped by x then.  "set": pic_set_particles uploads x and v as they are, without a refresh: the only way x = L,
a position outside the box or a non-finite one reaches phase_locate.  `particles(cid, load)` is what the kernels read."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

import hp_phase as hp

LD = np.longdouble
CEILING = 1e-9                # no bound is above this (hp_grad_cases.CEILING)
MARGIN = 100.0                # hp_grad_cases.MARGIN
TOL_KL, TOL_GRAD = 3.4e-14, 5.4e-14          # test_gpu_phase_kl.py
LDS_BYTES = 65536             # pic_phase.h: kPhaseLdsBytes


@dataclass(frozen=True)
class Case:
    id: str
    N: int
    nx: int
    nv: int
    E: int = 2
    L: float = 50.0
    n0: float = 1.0
    vmin: float = -6.0
    vmax: float = 6.0
    d_kl: tuple = (0.7, -1.3)

    def grid(self):
        return hp.Grid(self.nx, self.nv, self.L, self.vmin, self.vmax, self.N, self.n0)

    @property
    def rows(self):
        return rows(self.nx, self.nv)

    @property
    def bands(self):
        return -(-self.nx // self.rows)

    @property
    def boundaries(self):
        """The band boundaries whose positions are placed: the first four and the last."""
        return sorted(set(range(1, min(self.bands, 5))) | ({self.bands - 1} if self.bands > 1 else set()))


def rows(nx, nv):
    """Grid rows per band of the deposit (host_phase.h: phase_args)."""
    return min(nx, max(1, LDS_BYTES // (8 * nv)))


CASES = {c.id: c for c in (
    Case("A", 1, 1, 1),                                       # one particle, one bin, 61 weight bits
    Case("B", 2, 1, 7),                                       # nx = 1: both x bins are bin 0, g_x exactly 0
    Case("C", 3, 5, 1),                                       # nv = 1: every particle clamped, g_v exactly 0, odd N
    Case("D1", 255, 16, 16),                                  # abits + bbits = 54 ...
    Case("D2", 256, 16, 16),                                  # ... and 53
    Case("E", 257, 9, 1000),                                  # R = 8, two bands, the last of one row
    Case("F", 513, 1024, 1024),                               # 128 bands, LDS request exactly 64 KB
    Case("G", 4095, 250, 250, vmin=-2.0, vmax=3.0),           # partial last band, asymmetric range
    Case("H", 16385, 64, 3),                                  # three deposit workgroups; three forward-mode chunks, the last of one
    Case("I", 300, 33, 31, E=3, d_kl=(0.7, -1.3, 0.0)),       # env 1: every v above vmax; env 2 = env 0's particles
    Case("J", 1000, 33, 31, L=7.7, n0=4.0, vmin=0.5, vmax=0.5625),   # off-default constants, v - vmin near cancellation
)}
JVP_KS = {"D1": (1, 2, 4, 5, 8), "H": (1, 2, 4, 5, 8)}       # every other case: K = 3


def ks(cid):
    return JVP_KS.get(cid, (3,))


def positions(c):
    L, dx, R = c.L, c.L / c.nx, c.rows
    na = np.nextafter
    p = [0.0, -0.0, L, na(L, 0.0), na(0.0, 1.0), -1e-300, na(L, 2 * L)]
    for q in (dx / 2, L - dx / 2):
        p += [q, na(q, -np.inf), na(q, np.inf)]
    for b in c.boundaries:
        p += [b * R * dx, (b * R + 0.5) * dx, na((b * R + 0.5) * dx, -np.inf)]
    return p + [np.nan, np.inf]


def velocities(c):
    lo, hi = c.vmin, c.vmax
    dv = (hi - lo) / c.nv
    na = np.nextafter
    p = [lo, hi, na(lo, -np.inf), na(hi, np.inf), lo + dv / 2, hi - dv / 2, na(lo + dv / 2, -np.inf), na(hi - dv / 2, np.inf),
         lo + dv]
    if lo <= 0.0 <= hi:
        p.append(0.0)
    return p + [np.nan, np.inf, -np.inf]


@functools.lru_cache(maxsize=None)
def state(cid):
    """(X, V) [E, N] float64 of the case (see the module's docstring); never modified."""
    c = CASES[cid]
    rng = np.random.default_rng([c.N, c.nx, c.nv])
    w = 0.2 * (c.vmax - c.vmin)
    X = rng.uniform(0.0, c.L, (c.E, c.N))
    V = rng.uniform(c.vmin - w, c.vmax + w, (c.E, c.N))
    P, Q = positions(c), velocities(c)
    pairs = sorted(((i + j, i, j) for i in range(len(P)) for j in range(len(Q))))[:c.N]
    for k, (_, i, j) in enumerate(pairs):
        X[0, k], V[0, k] = P[i], Q[j]
    if cid == "I":
        V[1] = c.vmax + 0.1 + np.abs(V[1])              # all above vmax: dropped
        X[2], V[2] = X[0], V[0]
    X.setflags(write=False)
    V.setflags(write=False)
    return X, V


LOADS = ("reset", "set")


def fold(x, L):
    """np.mod(np.mod(x, L), L), a non-finite x parked at 0: the positions pic_reset's refresh stores (pic_device.h: wrap_periodic)."""
    with np.errstate(invalid="ignore"):
        r = np.mod(np.mod(x, L), L)
    return np.where(np.isfinite(r), r, 0.0) + 0.0


@functools.lru_cache(maxsize=None)
def particles(cid, load):
    """(X, V) [E, N] as the phase kernels read them after `load` (the module's docstring); never modified."""
    X, V = state(cid)
    if load == "reset":
        X = fold(X, CASES[cid].L)
        X.setflags(write=False)
    return X, V


def finite_state(cid, load):
    """The particles with every non-finite one replaced by a finite one outside the box (dropped as well)."""
    c = CASES[cid]
    X, V = (a.copy() for a in particles(cid, load))
    bad = ~(np.isfinite(X) & np.isfinite(V))
    X[bad], V[bad] = -1.0, c.vmax + 1.0
    return X, V


@functools.lru_cache(maxsize=None)
def targets(cid):
    """(shared [nx, nv], per environment [E, nx, nv]): uniform(0, 2 / (L (vmax - vmin))) with the bins [::3, ::2] exactly 0."""
    c = CASES[cid]
    rng = np.random.default_rng([c.N, c.nx, c.nv, 1])
    top = 2.0 / (c.L * (c.vmax - c.vmin))
    shared, per = rng.uniform(0.0, top, (c.nx, c.nv)), rng.uniform(0.0, top, (c.E, c.nx, c.nv))
    shared[::3, ::2] = 0.0
    per[:, ::3, ::2] = 0.0
    for a in (shared, per):
        a.setflags(write=False)
    return shared, per


@functools.lru_cache(maxsize=None)
def tangents(cid, K):
    """(d_x, d_v) [K, E, N] in [-1, 1]; case G's direction 1 (of K >= 2) scaled by 2^40."""
    c = CASES[cid]
    t = np.random.default_rng([c.N, c.nx, c.nv, 2, K]).uniform(-1.0, 1.0, (2, K, c.E, c.N))
    if cid == "G" and K >= 2:
        t[:, 1] *= 2.0 ** 40
    t.setflags(write=False)
    return t[0], t[1]


# ---- the longdouble reference ----------------------------------------------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.array(a, dtype=np.float64))          # (a copy: the cached inputs are read-only)


def _log_ratio(f, feq):
    """(pos, r): r = log(f / (feq + 1e-12)) in longdouble where f > 0 (0 elsewhere); f float64 [E, nx, nv]."""
    pos = f > 0
    y = np.broadcast_to(np.asarray(feq, dtype=LD) + LD(1e-12), f.shape)
    r = np.zeros(f.shape, dtype=LD)
    with np.errstate(divide="ignore"):
        r[pos] = np.log(f[pos].astype(LD) / y[pos])
    return pos, r


def kl_ld(X, V, G, feq):
    """(KL [E], S_kl [E]) in longdouble: sum f r dx dv over the bins with f > 0, and the condition scale sum |f r| dx dv."""
    f = hp.density(_t(X), _t(V), G).numpy()
    _, r = _log_ratio(f, feq)
    term = f.astype(LD) * r
    dxdv = LD(G.dx) * LD(G.dv)
    return term.sum(axis=(1, 2)) * dxdv, np.abs(term).sum(axis=(1, 2)) * dxdv


def vjp_ld(X, V, G, feq, d_kl):
    """(g_x, g_v) [E, N] in longdouble: the cotangent grid d (r + 1) dx dv gathered with hp_phase.locate's bins and fractions;
    exactly 0 for a dropped particle and in v without a slope."""
    f = hp.density(_t(X), _t(V), G).numpy()
    pos, r = _log_ratio(f, feq)
    g = np.where(pos, np.asarray(d_kl, dtype=LD)[:, None, None] * ((r + LD(1)) * (LD(G.dx) * LD(G.dv))), LD(0))
    inside, i0, i1, j0, j1, fx, fv, slope = (a.numpy() for a in hp.locate(_t(X), _t(V), G))
    fx, fv = fx.astype(LD), fv.astype(LD)
    gf = g.reshape(g.shape[0], -1)

    def at(i, j):
        return np.take_along_axis(gf, i * G.nv + j, axis=1)
    g00, g01, g10, g11 = at(i0, j0), at(i0, j1), at(i1, j0), at(i1, j1)
    gx = (LD(G.norm) * LD(G.rdx)) * ((g10 - g00) * (LD(1) - fv) + (g11 - g01) * fv)
    gv = (LD(G.norm) * LD(G.rdv)) * ((g01 - g00) * (LD(1) - fx) + (g11 - g10) * fx)
    return np.where(inside, gx, LD(0)), np.where(inside & slope, gv, LD(0))


def jvp_ld(gx, gv, d_x=None, d_v=None):
    """(sum_k gx_k dx_k + gv_k dv_k, S_jvp = sum_k |gx_k dx_k| + |gv_k dv_k|), each [K, E], in longdouble; gx, gv [E, N] of unit
    cotangents, d_x, d_v [K, E, N] or None (0)."""
    px = gx[None] * np.asarray(d_x, dtype=LD) if d_x is not None else LD(0)
    pv = gv[None] * np.asarray(d_v, dtype=LD) if d_v is not None else LD(0)
    out = np.sum(px + pv, axis=-1)
    return out, np.sum(np.abs(px) + np.abs(pv), axis=-1) + np.zeros_like(out)


@functools.lru_cache(maxsize=None)
def ref(cid, load):
    """The references of a case's particles after `load`, a dict: "f" [E, nx, nv] float64; "kl", "S_kl" [E] and "grad"
    (g_x, g_v) for the targets "shared" and "env" (cotangents c.d_kl); "unit" (g_x, g_v) of the per-environment target with unit
    cotangents, what the forward mode contracts with the tangents."""
    c = CASES[cid]
    X, V = particles(cid, load)
    G = c.grid()
    out = {"f": hp.density(_t(X), _t(V), G).numpy()}
    for name, feq in zip(("shared", "env"), targets(cid)):
        kl, S = kl_ld(X, V, G, feq)
        out[name] = {"kl": kl, "S_kl": S, "grad": vjp_ld(X, V, G, feq, c.d_kl)}
    out["unit"] = vjp_ld(X, V, G, targets(cid)[1], np.ones(c.E))
    return out


def ref_jvp(cid, load, K, which="both"):
    """(jvp_ld, S_jvp) [K, E] of the case's K tangents: d_x alone ("x"), d_v alone ("v") or both."""
    tx, tv = tangents(cid, K)
    return jvp_ld(*ref(cid, load)["unit"], tx if which != "v" else None, tv if which != "x" else None)


def grad_err(gx, gv, want):
    """max-abs error of (gx, gv) over the largest reference entry (1 if the reference is all zero)."""
    wx, wv = want
    scale = max(float(np.abs(wx).max()), float(np.abs(wv).max()))
    err = max(float(np.abs(np.asarray(gx, dtype=LD) - wx).max()), float(np.abs(np.asarray(gv, dtype=LD) - wv).max()))
    return err / scale if scale > 0 else err


def kl_err(kl, want, S):
    """max over the environments of |kl - want| / S_kl (environments with S_kl = 0 are held to exactly 0 by the caller)."""
    e = np.abs(np.asarray(kl, dtype=LD) - want)
    ok = S > 0
    return float((e[ok] / S[ok]).max()) if ok.any() else 0.0


@functools.lru_cache(maxsize=None)
def floors(cid, load):
    """The floor of a case: the float64 restatement against the longdouble reference, {"kl": hp_phase.kl over S_kl, "grad":
    hp_phase.vjp over the largest reference entry}, worst over the targets (and the unit cotangents).  Of the references alone."""
    c, r = CASES[cid], ref(cid, load)
    X, V = (_t(a) for a in particles(cid, load))
    G = c.grid()
    f = hp.density(X, V, G)
    fl = {"kl": 0.0, "grad": 0.0}
    for name, feq in zip(("shared", "env"), targets(cid)):
        fl["kl"] = max(fl["kl"], kl_err(hp.kl(f, _t(feq), G).numpy(), r[name]["kl"], r[name]["S_kl"]))
        gx, gv = hp.vjp(X, V, _t(feq), _t(c.d_kl), G)
        fl["grad"] = max(fl["grad"], grad_err(gx.numpy(), gv.numpy(), r[name]["grad"]))
    gx, gv = hp.vjp(X, V, _t(targets(cid)[1]), torch.ones(c.E, dtype=torch.float64), G)
    fl["grad"] = max(fl["grad"], grad_err(gx.numpy(), gv.numpy(), r["unit"]))
    return fl


def bound(cid, load, surface):
    """"kl": max(TOL_KL, 100 x floor); "grad": max(TOL_GRAD, 100 x floor); "jvp": 100 x gradient floor + N 2^-52 (the worst case
    of a float64 sum of 2N products in any order).  Never above the ceiling."""
    fl = floors(cid, load)
    b = {"kl": max(TOL_KL, MARGIN * fl["kl"]), "grad": max(TOL_GRAD, MARGIN * fl["grad"]),
         "jvp": MARGIN * fl["grad"] + CASES[cid].N * 2.0 ** -52}[surface]
    return min(b, CEILING)
