"""Bit-level restatement of the device sampler (csrc/pic_aux.h: sample_kernel, pic_reset_sampled).  TEST INFRASTRUCTURE ONLY.

Everything the kernel computes with IEEE operations under -ffp-contract=off is restated with the same float64 operations in
the same order, so its results are bit-identical: the Philox4x32-10 stream (in uint64 arithmetic), the key and counter
layout, u01, the population split, x and its per-format store.  The transcendental part of a velocity (log, sqrt, sincospi,
sin) is not correctly rounded on the device; `sample(..., ld=True)` evaluates it in np.longdouble from the same exact
arguments, and `velocity_bound` bounds the device's distance from that twin.
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
U32 = 2.0 ** -24
M32 = np.uint64(0xFFFFFFFF)
VMAX = 10.0                 # support of the reference's uniform proposal (dist.py:75)
ATTEMPTS = 63               # Box-Muller proposals per particle before the truncated-normal fallback


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Random123's Philox4x32-10 on arrays of uint64 holding 32-bit words; returns the four output words (uint64)."""
    c = [np.asarray(t, dtype=np.uint64) & M32 for t in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, dtype=np.uint64) & M32
    k1 = np.asarray(k1, dtype=np.uint64) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def u01(a, b):
    """((a << 21) ^ (b >> 11) + 0.5) 2^-53: in (0, 1], exactly 1.0 for the top bits (2^53 - 1 + 0.5 rounds to 2^53)."""
    bits = ((np.asarray(a, dtype=np.uint64) << np.uint64(21)) ^ (np.asarray(b, dtype=np.uint64) >> np.uint64(11)))
    return (bits.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def n_first(kind, N, a):
    """Particles of the first population: N / 2 (two-stream), int(N (1 / (1 + a))) bulk particles (bump-on-tail)."""
    return N // 2 if kind == 0 else int(float(N) * (1.0 / (1.0 + a)))


def key(seed, env):
    """(seed_lo ^ 0x85EBCA6B (env + 1), seed_hi) in 32-bit words; env is the global index env_base + e."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (seed & 0xFFFFFFFF) ^ ((0x85EBCA6B * ((env + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF), seed >> 32


def _fixed_from_length(xs, L):
    """pos_from_length<PosU32> (csrc/pic_device.h) in float64, bit for bit."""
    r = xs - np.floor(xs / L) * L
    r = np.where((r >= 0.0) & (r < L), r, 0.0)
    return (np.rint(r / L * 4294967296.0).astype(np.uint64) & M32).astype(np.uint32)


def sample(N, L, kind, a, v0, sigma, A, n_mode, seed, env, fmt="float64", ld=False):
    """One environment (global index env) of pic_reset_sampled.  Returns a dict:
      x          stored positions: float64 / float32 values, or uint32 fixed-point words (bit-identical to the device)
      v          velocities after the perturbation: float64 (ld=False, NumPy transcendentals) or longdouble (ld=True); not
                 rounded to the particle dtype
      v_raw      the same before the perturbation
      attempt    attempt that accepted (1..63), 64 for an exhausted draw
      mu, sg     mean and spread of each particle's population
      props      list over the attempts of (indices, proposal): every decision taken (decisions_near_edge)
      u_tail     the fallback's uniform (counter attempt 64), for every particle
      xs, arg    the float64 position before the store and the perturbation's sine argument
      r          sqrt(-2 log ua) of the accepted proposal (inf for exhausted draws)
    """
    i = np.arange(N, dtype=np.uint64)
    nf = n_first(kind, N, a)
    first = np.arange(N) < nf
    if kind == 0:
        mu = np.where(first, v0, -v0)
        sg = np.full(N, float(sigma))
    else:
        mu = np.where(first, 0.0, v0)
        sg = np.where(first, 1.0, float(sigma))
    k0, k1 = key(seed, env)
    lo, hi = i & M32, i >> np.uint64(32)
    c = philox4x32_10(lo, hi, 0, 0x50494331, k0, k1)
    xs = u01(c[0], c[1]) * L
    xs = np.where(xs >= L, 0.0, xs)
    ua = u01(c[2], c[3])
    T = LD if ld else np.float64
    vs = np.zeros(N, dtype=T)
    attempt = np.full(N, ATTEMPTS + 1, dtype=np.int64)
    r_acc = np.full(N, np.inf)
    props = []
    act = np.arange(N)
    for at in range(1, ATTEMPTS + 1):
        if act.size == 0:
            break
        d = philox4x32_10(lo[act], hi[act], at, 0x50494332, k0, k1)
        ang = 2.0 * u01(d[0], d[1])                                  # exact: the argument of sincospi
        if ld:
            r = np.sqrt(LD(-2) * np.log(ua[act].astype(LD)))
            cs = np.cos(ang.astype(LD) * (4 * np.arctan(LD(1))))
            p = LD(1) * mu[act] + (sg[act].astype(LD) * r) * cs
        else:
            p = mu[act] + sg[act] * np.sqrt(-2.0 * np.log(ua[act])) * np.cos(np.pi * ang)
        props.append((act, p))
        vs[act] = p
        ok = (p >= -VMAX) & (p <= VMAX)
        attempt[act[ok]] = at
        r_acc[act[ok]] = (np.sqrt(-2.0 * np.log(ua[act])))[ok]
        rej = act[~ok]
        ua[rej] = u01(d[2], d[3])[~ok]
        act = rej
    d = philox4x32_10(lo, hi, ATTEMPTS + 1, 0x50494332, k0, k1)
    u_tail = u01(d[0], d[1])
    v_raw = vs.copy()
    arg = 2.0 * 3.14159265358979323846 * n_mode * xs / L            # float64, the kernel's operand order
    if ld:
        v = vs * (LD(1) + LD(A) * np.sin(arg.astype(LD)))
    else:
        v = vs * (1.0 + A * np.sin(arg))
    if fmt == "float64":
        x = xs
    elif fmt == "float32":
        x = np.where(xs.astype(np.float32).astype(np.float64) >= L, 0.0, xs).astype(np.float32)
    else:
        x = _fixed_from_length(xs, L)
    return {"x": x, "v": v, "v_raw": v_raw, "attempt": attempt, "mu": mu, "sg": sg, "props": props, "u_tail": u_tail,
            "xs": xs, "arg": arg, "r": r_acc}


def proposal_bound(mu, g):
    """|device proposal - exact proposal| for mu + (sg sqrt(-2 log ua)) cs, g = sg sqrt(-2 log ua) cs (the twin's).
    log: <= 2 ulp (4 u64 relative), passed through -2 log and halved by sqrt: 2 u64; sqrt correctly rounded: u64; sincospi of
    the exact argument 2 u01: <= 2 ulp of |cs| (4 u64 relative: the reduction of its argument is exact); the products sg r and
    (sg r) cs: one rounding each.  So |dg| <= (2 + 1 + 4 + 2) u64 |g| (+ second order), and the sum with mu one rounding of
    the result: <= 10 u64 |g| + u64 (|mu| + |g|) + 2^-1074."""
    g = np.abs(np.asarray(g, dtype=np.float64))
    return 10 * U64 * g + U64 * (np.abs(mu) + g) + 5e-324


def velocity_bound(out, A, fmt):
    """|device v - twin v| for the particles whose decisions agree: the accepted proposal's bound (proposal_bound) and the
    absolute error of log near 1, then
    v (1 + A sin(arg)): sin of the exact float64 argument <= 2 ulp (4 u64 |sin| + 2^-1074), 1 + A s and the product one
    rounding each; then the store in the particle dtype, u_W of the result."""
    vr = np.abs(out["v_raw"].astype(np.float64))
    dv = proposal_bound(out["mu"], out["v_raw"].astype(np.float64) - out["mu"])
    # log(ua) for ua near 1 is accurate in absolute, not relative terms (|d log| <= 2^-60, say): through -2 log and sqrt
    # that is sg |cs| 2^-60 / r, r = sqrt(-2 log ua)
    dv = dv + out["sg"] * 2.0 ** -60 / np.maximum(out["r"], 1e-300)
    s = np.abs(np.sin(out["arg"]))
    fac = 1.0 + abs(A) * s
    dv = dv * fac + vr * (abs(A) * (4 * U64 * s + 5e-324) + 2 * U64 * fac)
    u = U64 if fmt == "float64" else U32
    return dv + u * vr * fac


def decisions_near_edge(out):
    """Particles for which some proposal the twin decided on (up to the accepted one) lies within proposal_bound of +-10:
    the device's rounded proposal may fall on the other side of the edge there, and its draw then continues (or stops)
    where the twin's does not."""
    amb = np.zeros(out["mu"].size, dtype=bool)
    for idx, p in out["props"]:
        pf = np.asarray(p, dtype=np.float64)
        b = proposal_bound(out["mu"][idx], pf - out["mu"][idx])
        amb[idx] |= np.abs(np.abs(pf) - VMAX) <= b
    return amb
