"""Extended-precision restatement of the reference's step.  TEST INFRASTRUCTURE ONLY.

Everything here runs in NumPy ``np.longdouble`` (x87 80-bit: a 64-bit mantissa, unit roundoff 5.4e-20), so that its own
rounding is three orders of magnitude below the float64 arithmetic it checks.  It restates the same operations as
``oracle/pic_oracle.py`` (citations relative to the reference's tree, as there), with two deliberate differences:

* the periodic Poisson problem is solved by cumulative sums with a mean-zero gauge (the formulation of
  ``csrc/pic_device.h: scan_fields``), not by the reference's Sherman-Morrison elimination (``solve.py:27-53``), whose
  denominator is exactly zero for many ``(L, Ng)`` pairs.  Where the reference is defined the two agree (tests/test_hp_reference.py);
* densities are deposited with the exact shape weights of the given positions, accumulated with ``np.add.at`` on
  longdouble arrays (``np.bincount`` would cast the weights to float64).

The functions take the device's own state and return what one stage of the reference makes of it, so that the GPU tests can
check a step stage by stage (tests/test_gpu_local_parity.py).
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "hp_reference needs an extended-precision np.longdouble (x87 80-bit or binary128)"

TWO32 = LD(2) ** 32
PI = 4 * np.arctan(LD(1))


def as_ld(a):
    return np.asarray(a).astype(LD)


def wrap(q, L):
    """np.mod(np.mod(q, L), L): PIC.update_state (pic.py:139), then compute_n (util.py:51) before CIC / TSC wraps its copy
    (interpolate.py:6).  In longdouble the remainder is exact."""
    L = LD(L)
    return np.mod(np.mod(as_ld(q), L), L)


def fixed_to_length(u, L):
    """Exact position of a 32-bit fixed-point coordinate: x = u L / 2^32 (torch_views()["x_fixed"] holds u's bits)."""
    u = np.asarray(u).astype(np.int64) & 0xFFFFFFFF
    return u.astype(LD) * LD(L) / TWO32


def fixed_from_length(x, L):
    """The 32-bit fixed-point image of lengths x: round(mod(x, L) / L 2^32) mod 2^32, the remainder exact in longdouble and
    one rounding to the 2^-32 grid (ties to even).  Finite x only."""
    L = LD(L)
    r = np.mod(as_ld(x), L)
    return (np.rint(r / L * TWO32).astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def yoshida4_coefficients():
    """The reference's float64 coefficients (integration.py:62-75), carried exactly into longdouble."""
    cbrt2 = 2 ** (1 / 3)
    w0 = (-1) * cbrt2 / (2 - cbrt2)
    w1 = 1 / (2 - cbrt2)
    c1 = 0.5 * w1
    c2 = 0.5 * (w0 + w1)
    return (LD(c1), LD(c2), LD(c2), LD(c1)), (LD(0), LD(w1), LD(w0), LD(w1))


def _cells(x, Ng, L, cell_dtype=None):
    """Leftmost cell index jf (unfolded, as floor(xw / dx)) and the exact offset d = xw / dx - jf in cells.

    x of dtype uint32: fixed-point positions, jf = floor(u Ng / 2^32) and d = (u Ng mod 2^32) / 2^32, both exact.
    Otherwise x is a length; it is wrapped exactly, and jf follows the index rule interpolate.py:7 / :25 in the given
    floating-point dtype (np.floor(xw / dx) with that dtype's IEEE division and dx = L / Ng rounded to it), or with exact
    division when cell_dtype is None.  d is exact either way; it lies slightly outside [0, 1) where the dtype's rounded
    quotient crosses a cell edge the exact one does not.  Both shape functions are polynomials in d once the cell is fixed.
    """
    x = np.asarray(x)
    if x.dtype == np.uint32:
        t = x.astype(np.uint64) * np.uint64(Ng)
        jf = (t >> np.uint64(32)).astype(np.int64)
        d = (t & np.uint64(0xFFFFFFFF)).astype(LD) / TWO32
        return jf, d
    xw = wrap(x, L)
    dx = LD(L) / LD(Ng)
    if cell_dtype is None:
        jf = np.floor(xw / dx).astype(np.int64)
    else:
        dt = np.dtype(cell_dtype)
        dxw = dt.type(float(L) / Ng)
        jf = np.floor(xw.astype(dt) / dxw).astype(np.int64)
    return jf, xw / dx - jf.astype(LD)


def shape_weights(d, shape):
    """(node offsets, weights [k][N]) relative to jf: CIC interpolate.py:9-12, TSC interpolate.py:26-34."""
    if shape == "CIC":
        return (0, 1), np.stack([1 - d, d])
    half, tq = LD(0.5), LD(0.75)
    return (-1, 0, 1), np.stack([half * (LD(1.5) - d) ** 2, tq - (d - 1) ** 2, half * (d - half) ** 2])


def deposit(x, Ng, L, n0, N, shape="CIC", cell_dtype=None):
    """Density (interpolate.py:4-44, util.py:48-70) with the exact weights of the positions x (lengths, or uint32 fixed point),
    scaled by n0 L / N / dx (interpolate.py:18).  Returns (n [Ng] longdouble, count [Ng]): count_j = particles whose shape
    touches node j."""
    jf, d = _cells(x, Ng, L, cell_dtype)
    offs, w = shape_weights(d, shape)
    n = np.zeros(Ng, dtype=LD)
    count = np.zeros(Ng, dtype=np.int64)
    for o, wk in zip(offs, w):
        nodes = np.mod(jf + o, Ng)
        np.add.at(n, nodes, wk)
        count += np.bincount(nodes, minlength=Ng)
    dx = LD(L) / LD(Ng)
    return n * (LD(n0) * LD(L) / LD(N) / dx), count


def solve(n, n0, L):
    """3-point periodic Poisson solve with a mean-zero gauge (pic.py:114-117, solve.py:27-53, util.py:99-103), by cumulative
    sums as csrc/pic_device.h:scan_fields does it: G_{j+1/2} = dx cumsum(n - n0), minus its mean; E_j = -(G_{j+1/2} +
    G_{j-1/2}) / 2; phi_{j+1} = phi_j + dx G_{j+1/2}, minus its mean.  -> (E_mesh, phi), without any external field."""
    b = as_ld(n) - LD(n0)
    Ng = b.size
    dx = LD(L) / LD(Ng)
    G = np.cumsum(b) * dx
    G = G - np.sum(G) / LD(Ng)
    E = LD(-0.5) * (G + np.roll(G, 1))
    phi = np.concatenate([np.zeros(1, dtype=LD), np.cumsum(G[:-1] * dx)])
    phi = phi - np.sum(phi) / LD(Ng)
    return E, phi


def gather(E_mesh, x, L, shape="CIC", cell_dtype=None):
    """The mesh field at the particles with the deposit's cells and weights (pic.py:118-123)."""
    E_mesh = as_ld(E_mesh).ravel()
    Ng = E_mesh.size
    jf, d = _cells(x, Ng, L, cell_dtype)
    offs, w = shape_weights(d, shape)
    out = np.zeros(jf.shape, dtype=LD)
    for o, wk in zip(offs, w):
        out += wk * E_mesh[np.mod(jf + o, Ng)]
    return out


def yoshida4_step(x, v, E_ext, dt, Ng, L, n0, N, shape="CIC", cell_dtype=None):
    """One update_state (pic.py:131-146) in the operand order of OraclePIC._lean_step: per sub-stage (c, d), kick
    p += (d (-E)) dt with E the field of the current positions (+ E_ext), then drift q += (c p) dt; the final positions
    wrapped.  x: lengths or uint32 fixed point (the state before the step); cells of the sub-stage positions by the rule
    of cell_dtype (see _cells).  Returns (x_new, v_new, info) with info["q"] [4][N] the unwrapped positions after each drift,
    info["p"] [4][N] the velocities after each kick, info["E"] [(sub-stage, E_mesh + E_ext, E at particles, n, count)] of
    the three force evaluations."""
    q = fixed_to_length(x, L) if np.asarray(x).dtype == np.uint32 else as_ld(x)
    p = as_ld(v)
    dt = LD(dt)
    ext = None if E_ext is None else as_ld(E_ext).ravel()
    cs, ds = yoshida4_coefficients()
    info = {"q": [], "p": [], "E": []}
    for s, (c, d) in enumerate(zip(cs, ds)):
        if d != 0:
            n, count = deposit(q, Ng, L, n0, N, shape, cell_dtype)
            E, _ = solve(n, n0, L)
            if ext is not None:
                E = E + ext
            Ep = gather(E, q, L, shape, cell_dtype)
            p = p + d * (-Ep) * dt
            info["E"].append((s, E, Ep, n, count))
        info["p"].append(p)
        q = q + c * p * dt
        info["q"].append(q)
    return wrap(q, L), p, info


def energies(v, E_mesh, L, N):
    """(KE, PE, PE_reward): 0.5 sum(v^2) (util.py:144), 0.5 sum(E^2) dx N / L (util.py:129-130) and 0.5 sum(E^2) dx
    (objective.py:33), summed in longdouble."""
    v = as_ld(v)
    E = as_ld(E_mesh).ravel()
    dx = LD(L) / LD(E.size)
    ke = LD(0.5) * np.sum(v * v)
    per = LD(0.5) * np.sum(E * E) * dx
    return ke, per * LD(N) / LD(L), per


def modes(E_mesh, M):
    """fft(E)[m] / Ng * 2 for m = 1..M (spectrum.py:16) by a direct DFT in longdouble; the angle 2 pi m j / Ng is reduced
    modulo 2 pi in integers first."""
    E = as_ld(E_mesh).ravel()
    Ng = E.size
    j = np.arange(Ng, dtype=np.int64)
    re = np.zeros(M, dtype=LD)
    im = np.zeros(M, dtype=LD)
    for m in range(1, M + 1):
        ang = LD(2) * PI * ((m * j) % Ng).astype(LD) / LD(Ng)
        re[m - 1] = np.sum(E * np.cos(ang)) / LD(Ng) * 2
        im[m - 1] = -np.sum(E * np.sin(ang)) / LD(Ng) * 2
    return re, im


def feedback_action(E_mesh, M):
    """The linear feedback law of run_feedback.py:133-135: cos coefficients -Re E_k, sin coefficients +Im E_k."""
    re, im = modes(E_mesh, M)
    return np.concatenate([-re, im])
