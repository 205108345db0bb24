"""Extended-precision restatement of the reference's other integrators.  TEST INFRASTRUCTURE ONLY.

One PIC.update_state (pic.py:131-146) with `symplectic_4th_order` replaced by symplectic_euler (integration.py:50), verlet (:54)
or forward_euler (:8), in ``np.longdouble`` on top of tests/hp_reference.py's deposit, solve and gather (imported, not edited).
Operand order as the reference's: kick p + (d (-E)) dt, drift q + (c p) dt, forward Euler eta + dt grad(eta); a zero
coefficient skips its kick or drift.
"""
import numpy as np

from hp_reference import LD, as_ld, deposit, fixed_to_length, gather, solve, wrap

SCHEMES = ("symplectic_euler", "verlet", "forward_euler")
EVALS = {"symplectic_euler": 1, "verlet": 2, "forward_euler": 1}


def force(q, E_ext, Ng, L, n0, N, shape="CIC", cell_dtype=None, info=None):
    """-> (E at the particles, E_mesh + E_ext): the field of the deposit of q (compute_E, util.py:73-116).  info: appends
    (E_mesh + E_ext, E at the particles, n, count) to info["E"]."""
    n, count = deposit(q, Ng, L, n0, N, shape, cell_dtype)
    E, _ = solve(n, n0, L)
    if E_ext is not None:
        E = E + as_ld(E_ext).ravel()
    Ep = gather(E, q, L, shape, cell_dtype)
    if info is not None:
        info["E"].append((E, Ep, n, count))
    return Ep, E


def scheme_step(scheme, x, v, E_ext, dt, Ng, L, n0, N, shape="CIC", cell_dtype=None):
    """One step of `scheme` from (x, v) (lengths, or uint32 fixed point).  -> (x_new wrapped, v_new, info) with info["q"] the
    unwrapped positions after each drift, info["p"] the velocities after each kick and info["E"] what `force` appends."""
    q = fixed_to_length(x, L) if np.asarray(x).dtype == np.uint32 else as_ld(x)
    p = as_ld(v)
    dt = LD(dt)
    info = {"q": [], "p": [], "E": []}
    if scheme == "forward_euler":
        q = wrap(q, L)                                   # grad_func wraps eta's positions in place (util.py:51)
        Ep, _ = force(q, E_ext, Ng, L, n0, N, shape, cell_dtype, info)
        q, p = q + dt * p, p + dt * (-Ep)
        info["q"].append(q)
        info["p"].append(p)
    elif scheme == "symplectic_euler":
        Ep, _ = force(q, E_ext, Ng, L, n0, N, shape, cell_dtype, info)
        p = p + LD(1) * (-Ep) * dt
        q = q + LD(1) * p * dt
        info["p"].append(p)
        info["q"].append(q)
    elif scheme == "verlet":
        for c, d in ((LD(1), LD(0.5)), (LD(0), LD(0.5))):
            Ep, _ = force(q, E_ext, Ng, L, n0, N, shape, cell_dtype, info)
            p = p + d * (-Ep) * dt
            info["p"].append(p)
            if c != 0:
                q = q + c * p * dt
                info["q"].append(q)
    else:
        raise ValueError(scheme)
    return wrap(q, L), p, info


def run(scheme, x, v, steps, dt, Ng, L, n0, N, shape="CIC", E_ext=None):
    """`steps` steps (E_ext: None, one field for all steps, or a list of one per step) -> list of (x, v) after each step."""
    out = []
    for k in range(steps):
        e = E_ext[k] if isinstance(E_ext, list) else E_ext
        x, v, _ = scheme_step(scheme, x, v, e, dt, Ng, L, n0, N, shape)
        out.append((x, v))
    return out
