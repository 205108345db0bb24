"""Stage checks of a device step against tests/hp_reference.py (longdouble), with bounds derived from the arithmetic.
TEST INFRASTRUCTURE ONLY, shared by the GPU test files.

`check_stages` compares the state a step left (density, E_mesh, phi, energies) with the reference evaluated on that state;
`check_push` compares the step itself with hp_reference.yoshida4_step from the device's state before it.  Every bound is a
formula with its derivation next to it (`density_bound`, `solve_bounds`, `push_bound`, `energy_bounds`), and every measured /
bound ratio is recorded with record_measure.
"""
import numpy as np

import hp_reference as hp
from conftest import record_measure

U64 = 2.0 ** -53          # unit roundoff, float64
U32 = 2.0 ** -24          # unit roundoff, float32
LD = hp.LD


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, dtype, pos, shape, N, Ng, L, envs=1, accum=None, bpe=0, ext=False, actions=False, planted=None,
                 n0=1.0, dt=0.05, steps=2, check_envs=1, sampled=False):
        self.dtype, self.pos, self.shape, self.N, self.Ng, self.L = dtype, pos, shape, N, Ng, L
        self.envs, self.accum, self.bpe, self.ext, self.actions, self.planted = envs, accum, bpe, ext, actions, planted
        self.n0, self.dt, self.steps, self.check_envs, self.sampled = n0, dt, steps, min(check_envs, envs), sampled

    @property
    def fixed(self):
        return self.pos == "fixed32"

    def __repr__(self):
        return (f"{self.dtype}/{self.pos}/{self.shape}/acc={self.accum}/bpe={self.bpe} envs={self.envs} N={self.N} "
                f"Ng={self.Ng} L={self.L} ext={self.ext} act={self.actions} planted={self.planted}")




def _planted_positions(c, rng):
    """Positions on and next to the edges the index rule and the wrap can get wrong: +-0, L - ulp, tiny negatives, k dx
    and its two neighbours (in the particle dtype)."""
    W = np.dtype(c.dtype).type
    L = W(c.L)
    dx = W(c.L / c.Ng)
    k = rng.integers(0, c.Ng, 24)
    kd = (k.astype(c.dtype) * dx).astype(c.dtype)
    edge = [W(0.0), W(-0.0), np.nextafter(L, W(0)), W(-1e-30), -np.nextafter(W(0), W(1)), W(-1e-7 * c.L * 1e-9)]
    pts = np.concatenate([np.array(edge, dtype=c.dtype), kd, np.nextafter(kd, W(c.L)), np.nextafter(kd, W(-1))])
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------
def _fg(N):
    """Fractional bits of the 64-bit accumulators, as pic_create computes them (csrc/picstep.hip:1096-1099)."""
    lg = 0
    while (1 << lg) < N + 1:
        lg += 1
    return min(50, 62 - lg)


def _acc_kind(c):
    if c.accum in (None, "auto"):
        return "packed" if (c.dtype == "float32" and c.shape == "CIC") else "fix64"
    return "packed" if c.accum in ("fixed", "packed") else c.accum


def _u(c):
    return U64 if c.dtype == "float64" else U32


def gather_bound(c, E_mesh):
    """|gathered - sum_k w_k(exact) E_mesh[node_k]| for the device's gather (csrc/pic_device.h: gather_field) from the mesh
    E_mesh it holds, at one particle.  The device computes in the particle dtype W (float for float32 and fixed32 particles):
      the mesh tile is E_mesh cast to W: |dE_k| <= u_W |E_k|, times sum|w| <= 1 + n_w w_err;
      each weight is off by w_err (_weight_err): n_w w_err max|E|;
      n_w products and n_w - 1 additions in W, recursive summation: (2 n_w - 1) u_W sum|w_k E_k| (+ second order).
    With the particle dtype's store of the result (exact: the sum is already in W):
      |dE_p| <= max|E| (n_w w_err + (1 + n_w w_err) u_W + 2 n_w u_W)."""
    nw = 2 if c.shape == "CIC" else 3
    we = _weight_err(c)
    uw = _u(c)
    return float(np.max(np.abs(E_mesh))) * (nw * we + (1 + nw * we) * uw + 2 * nw * uw)


def _weight_err(c):
    """Error of one device shape weight against the exact weight of the same stored position.
    Float positions: d = (xw - jf dx_W) / dx_W in the particle dtype W.  dx_W = fl(L / Ng) is off by u_W relative, so jf dx_W
    is off by up to jf dx u_W <= L u_W = Ng u_W cells, and the rounding of the product jf dx_W (<= L) adds as much again; the
    difference and the division (div_dx, with dx_W's error once more) add 3 u_W: |delta d| <= (2 Ng + 4) u_W.  CIC weights
    have slope 1 in d, TSC weights at most 2; the weight polynomial adds 3 u_W.
    Fixed point: d = float(frac) 2^-32 is d rounded once, the polynomial adds a few u_32, whatever Ng."""
    k = 1 if c.shape == "CIC" else 2
    u = _u(c)
    if c.fixed:
        return (k + 3) * u
    return (k * (2 * c.Ng + 4) + 3) * u


def _quantum(c):
    """Rounding of one weight by the accumulator.
    fix64: round(w 2^fg), half a unit.  float64: float64 running sums, flushed to 2^-fg units once per workgroup (one half
    unit, at most one per particle) plus count_j u64 per add (added by density_bound).  packed: w_r rounded to 2^-24: from
    the fixed-point fraction (frac >> 8) + carry, half a unit; from a float weight (float)(w_r 2^24 + 0.5) truncated, where
    w_r 2^24 + 0.5 is itself rounded to float32 -- for w_r >= 0.5 that rounds half to even, i.e. up to one whole unit."""
    kind = _acc_kind(c)
    if kind == "packed":
        return 2.0 ** -25 if c.fixed else 2.0 ** -24
    return 2.0 ** -(_fg(c.N) + 1)


def density_bound(c, n_hp, count):
    """|n_dev - n_hp|_j <= count_j (weight error + quantum [+ count_j u64 for float64 running sums]) scale + 6 u64 |n_j|:
    the last term is the conversion (double)acc, the scale n0 L / N / dx (four roundings on the host) and its product."""
    scale = c.n0 * c.L / c.N / (c.L / c.Ng)
    per = _weight_err(c) + _quantum(c)
    cnt = count.astype(float)
    if _acc_kind(c) == "float64":
        per = per + cnt * U64
    return cnt * per * scale + 6 * U64 * np.abs(n_hp.astype(float))


def solve_bounds(c, n_dev, E_dev):
    """Rounding of the device's solve (csrc/pic_device.h:scan_fields, solve_block) of its own density b = fl(n - n0).
    Prefix sums: each lane adds its m = ceil(Ng / 64) nodes, 6 DPP steps carry the lane totals, the lane adds its nodes
    again: at most 2m + 6 additions on any path, each off by u64 of a partial sum <= sum|b|; with b's own rounding and the
    product by dx, |dG| <= (2m + 8) u64 dx sum|b|.  The mean of G (m + 7 additions and a division) and the two differences
    of E = -(G_j+ + G_j-) / 2 add (m + 10) u64 max|G| <= (m + 10) u64 dx sum|b|.  So
    |E_dev - E_hp| <= (5m + 26) u64 dx sum|b| + u64 max|E|.
    phi_j = sum_{i<j} (G_i - gmean) dx: Ng terms each off by 2 |dG|, the second scan's own 2m + 9 roundings of partial sums
    of |G| dx, and the mean removal doubles it: |dphi| <= 2 (2 L |dG| + (2m + 9) u64 dx sum|G|) + u64 max|phi|."""
    Ng = c.Ng
    m = (Ng + 63) // 64
    dx = c.L / Ng
    b = np.abs(n_dev - c.n0)
    sb = float(np.sum(b)) * dx
    dG = (2 * m + 8) * U64 * sb
    bE = (5 * m + 26) * U64 * sb + U64 * float(np.max(np.abs(E_dev)))
    G = np.cumsum(n_dev - c.n0) * dx
    G -= G.mean()
    bphi = 2 * (2 * c.L * dG + (2 * m + 9) * U64 * dx * float(np.sum(np.abs(G))))
    return bE, bphi, dG


def energy_bounds(c, ke, per):
    """KE = 0.5 sum v^2 over N terms and PE_reward = 0.5 sum E^2 dx over Ng terms, summed in float64 in some order: at most
    (terms + 64) u64 relative (recursive summation); PE = PE_reward N / L two roundings more."""
    bke = (c.N + 64) * U64 * float(ke)
    bper = (c.Ng + 64) * U64 * float(per)
    return bke, bper, (c.Ng + 66) * U64 * float(per) * c.N / c.L


# ---------------------------------------------------------------------------------------------------------------------
# device state
# ---------------------------------------------------------------------------------------------------------------------
def _read(env, c, e, views):
    """Exact state of environment e: positions (uint32 bit patterns for fixed point), velocities, fields, energies."""
    env.sync()
    if c.fixed:
        x = views["x_fixed"][e].cpu().numpy().view(np.uint32).copy()
    else:
        x = views["x"][e].cpu().numpy().copy()
    v = views["v"][e].cpu().numpy().copy()
    st = {"x": x, "v": v}
    for k in ("n", "E_mesh", "phi"):
        st[k] = views[k][e].cpu().numpy().copy()
    for k in ("KE", "PE", "PE_reward"):
        st[k] = float(views[k][e].cpu())
    return st


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------
_WORST = {}


def _ratio(name, value, bound):
    r = float(value) / float(bound) if bound > 0 else (0.0 if value == 0 else np.inf)
    _WORST[name] = max(_WORST.get(name, 0.0), r)
    record_measure("local_parity_" + name, _WORST[name])
    return r


def _cell_dtype(c):
    return None if c.fixed else np.dtype(c.dtype)


def check_stages(c, st, tag):
    """n against the deposit of the stored positions; E_mesh and phi against the solve of the device's own n; the energies
    against the sums of the device's own v and E_mesh."""
    n_hp, count = hp.deposit(st["x"], c.Ng, c.L, c.n0, c.N, c.shape, _cell_dtype(c))
    bn = density_bound(c, n_hp, count)
    dn = np.abs(st["n"] - n_hp).astype(float)
    assert np.all(dn <= bn), (tag, "n", float(np.max(dn / np.maximum(bn, 1e-300))))
    _ratio("n", np.max(dn / np.maximum(bn, 1e-300)), 1.0)
    E_hp, phi_hp = hp.solve(st["n"], c.n0, c.L)
    bE, bphi, _ = solve_bounds(c, st["n"], st["E_mesh"])
    eE = float(np.max(np.abs(st["E_mesh"] - E_hp)))
    assert eE <= bE, (tag, "E_mesh", eE, bE)
    _ratio("E_mesh", eE, bE)
    phi = st["phi"] - np.mean(st["phi"].astype(LD))
    ephi = float(np.max(np.abs(phi - phi_hp)))
    bphi += U64 * float(np.max(np.abs(phi_hp)))
    assert ephi <= bphi, (tag, "phi", ephi, bphi)
    _ratio("phi", ephi, bphi)
    ke, pe, per = hp.energies(st["v"], st["E_mesh"], c.L, c.N)
    bke, bper, bpe = energy_bounds(c, ke, per)
    for name, dev, ref, b in (("KE", st["KE"], ke, bke), ("PE_reward", st["PE_reward"], per, bper), ("PE", st["PE"], pe, bpe)):
        err = abs(float(LD(dev) - ref))
        assert err <= b + 1e-300, (tag, name, err, b)
        _ratio(name, err, b)
    return n_hp, count


def push_bound(c, pre, info, E_ext_err):
    """Per-particle bounds (dx, dv) on the device's step from `pre` against hp.yoshida4_step from the same state.
    Sub-stage s (kick with d_s, then drift with c_s), errors carried from the previous sub-stage as dq, dp:
      field on the mesh: the device deposits its own sub-stage positions (off by dq: CIC weights have slope 1 / dx, TSC 2 / dx)
        with the weight / accumulator errors of density_bound; dn_j <= count_j (w_err + q + Lip dq / dx) scale + 6 u64 |n|;
        TSC only: a particle within the rounding window of a cell edge may be put in the neighbouring cell, where the
        reference's TSC weights jump (they are not continuous at the edges): 3 scale on each of its 5 nodes.
        The solve is linear: |dE_mesh| <= 2 dx sum_j dn_j (cumulative sum, gauge, average) + its own rounding (solve_bounds)
        + the external field's (actuator tables summed on the device in another order: E_ext_err).
      at the particle: sum_k |w_k| (<= 1.6) |dE_mesh| + max|E| (n_w |dw| + (2 n_w + 2) u_W) (+ 3 max|E| for a TSC particle
        in an edge window);
      kick  p + (d (-E)) dt in W:   dp += |d| dt dE_p + 4 u_V (|p| + |d E_p dt|);
      drift q + (c p) dt in W:      dq += |c| dt dp + 4 u_X (|q| + |c p dt|); fixed point instead 4 u_32 |c p dt| + L 2^-33
                                    (the displacement rounded to position units).
    The final wrap is exact (fmod; q - L by Sterbenz) except q + L for a tiny negative q: u_X L."""
    u = _u(c)
    cs, ds = hp.yoshida4_coefficients()
    dt = float(c.dt)
    dx = c.L / c.Ng
    scale = c.n0 * c.L / c.N / dx
    nw = 2 if c.shape == "CIC" else 3
    lip = 1.0 if c.shape == "CIC" else 2.0
    wsum = 1.0 if c.shape == "CIC" else 1.6
    N = pre["v"].size
    dq = np.zeros(N)
    dp = np.zeros(N)
    q_prev = hp.fixed_to_length(pre["x"], c.L) if c.fixed else hp.as_ld(pre["x"])
    E_iter = iter(info["E"])
    for s in range(4):
        if float(ds[s]) != 0.0:
            _, Em, Ep, n_hp, count = next(E_iter)
            dqmax = float(np.max(dq))
            per = _weight_err(c) + _quantum(c) + lip * dqmax / dx
            cnt = count.astype(float)
            if _acc_kind(c) == "float64":
                per = per + cnt * U64
            dn = cnt * per * scale + 6 * U64 * np.abs(n_hp.astype(float))
            amb = np.zeros(N, dtype=bool)
            if c.shape == "TSC":
                qc = hp.wrap(q_prev, c.L) / LD(dx)
                dist = np.abs(qc - np.round(qc)).astype(float)
                amb = dist <= (dq / dx + (2 * c.Ng + 4) * u + 1e-15)
                if amb.any():
                    jf = np.floor(qc[amb]).astype(np.int64)
                    for o in (-2, -1, 0, 1, 2):
                        np.add.at(dn, np.mod(jf + o, c.Ng), 3.0 * scale)
            Emax = float(np.max(np.abs(Em)))
            m = (c.Ng + 63) // 64
            sb = float(np.sum(np.abs(n_hp.astype(float) - c.n0))) * dx + float(np.sum(dn)) * dx
            dE_mesh = 2 * dx * float(np.sum(dn)) + (5 * m + 26) * U64 * sb + 2 * U64 * Emax + E_ext_err
            dEp = wsum * dE_mesh + Emax * (nw * (_weight_err(c) + lip * dq / dx) + (2 * nw + 2) * u)
            dEp = dEp + np.where(amb, 3.0 * Emax, 0.0)
            p = np.abs(info["p"][s].astype(float))
            kick = np.abs(float(ds[s]) * Ep.astype(float) * dt)
            dp = dp + abs(float(ds[s])) * dt * dEp + 4 * u * (p + kick)
        p = np.abs(info["p"][s].astype(float))
        q = np.abs(info["q"][s].astype(float))
        drift = abs(float(cs[s])) * p * dt
        if c.fixed:
            dq = dq + abs(float(cs[s])) * dt * dp + 4 * U32 * drift + c.L * 2.0 ** -33
        else:
            dq = dq + abs(float(cs[s])) * dt * dp + 4 * u * (q + drift)
        q_prev = info["q"][s]
    if not c.fixed:
        dq = dq + u * c.L
    return dq, dp


def check_push(c, pre, post, E_ext, E_ext_err, tag, skip=None):
    x1, v1, info = hp.yoshida4_step(pre["x"], pre["v"], E_ext, c.dt, c.Ng, c.L, c.n0, c.N, c.shape, _cell_dtype(c))
    bq, bp = push_bound(c, pre, info, E_ext_err)
    xd = hp.fixed_to_length(post["x"], c.L) if c.fixed else hp.as_ld(post["x"])
    d = np.abs(xd - x1)
    d = np.minimum(d, LD(c.L) - d).astype(float)
    dv = np.abs(hp.as_ld(post["v"]) - v1).astype(float)
    ok = np.ones(d.size, dtype=bool) if skip is None else ~skip
    assert np.all(d[ok] <= bq[ok]), (tag, "x", float(np.max(d[ok] / bq[ok])))
    assert np.all(dv[ok] <= bp[ok]), (tag, "v", float(np.max(dv[ok] / bp[ok])))
    _ratio("x", np.max(d[ok] / bq[ok]), 1.0)
    _ratio("v", np.max(dv[ok] / bp[ok]), 1.0)


def check_energies_of(c, x, v, ke_dev, pe_dev, per_dev, tag):
    """The energies a multi-step call recorded after an inner step, against the reference's energies of that step's state
    (taken from the single-stepping twin): density bound -> field bound |dE| <= 2 dx sum dn + solve rounding ->
    |dPE_r| <= dx sum_j (|E_j| + |dE| / 2) |dE| + summation rounding."""
    n_hp, count = hp.deposit(x, c.Ng, c.L, c.n0, c.N, c.shape, _cell_dtype(c))
    E_hp, _ = hp.solve(n_hp, c.n0, c.L)
    ke, pe, per = hp.energies(v, E_hp, c.L, c.N)
    dx = c.L / c.Ng
    dn = density_bound(c, n_hp, count)
    m = (c.Ng + 63) // 64
    dE = 2 * dx * float(np.sum(dn)) + (5 * m + 26) * U64 * (float(np.sum(np.abs(n_hp - c.n0))) * dx) + U64 * float(np.max(np.abs(E_hp)))
    bke, bper, _ = energy_bounds(c, ke, per)
    bper = bper + dx * float(np.sum(np.abs(E_hp.astype(float)) + dE / 2)) * dE
    for name, dev, ref, b in (("KE", ke_dev, ke, bke), ("PE_reward", per_dev, per, bper),
                              ("PE", pe_dev, pe, bper * c.N / c.L * (1 + 4 * U64))):
        err = abs(float(LD(dev) - ref))
        assert err <= b + 1e-300, (tag, "multi-step " + name, err, b)
        _ratio("multistep_" + name, err, b)


def check_handle_step(env, dtype, pos, shape, E_ext=None, accum=None, tag=""):
    """One more single step of an existing handle, checked step-locally in every environment: check_push from the state before
    it, check_stages of the state after it.  E_ext: [num_envs, Ng] or None."""
    c = Case(dtype, pos or "float", shape, env.N, env.N_mesh, env.L, env.num_envs, accum, n0=env.n0, dt=env.dt)
    views = env.torch_views()
    pre = [_read(env, c, e, views) for e in range(env.num_envs)]
    env.step(E_ext, 1)
    for e in range(env.num_envs):
        post = _read(env, c, e, views)
        t = f"{tag} {c} env {e}"
        check_stages(c, post, t)
        check_push(c, pre[e], post, None if E_ext is None else E_ext[e], 0.0, t)
