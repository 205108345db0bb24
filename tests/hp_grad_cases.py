"""The edge-shape matrix of the differentiation stack (last paragraph).  TEST INFRASTRUCTURE ONLY.

The case table, the inputs of every case, and the float64 references of tests/hp_*.py evaluated on them once per process: shared
by tests/test_grad_edges_cpu.py (the premises, on the references alone) and tests/test_gpu_grad_edges.py (the device).

Inputs of environment e of a case, all from np.random.default_rng([N, Ng, salt, e]) in this order: x = uniform(0, L, N),
v = normal(0, 0.03 L, N), ext = 0.05 standard_normal((T, Ng)), then standard normal cotangents (energies [T, 3], x_T, v_T [N],
KL [T], moments [T, 3, Ng]) and tangents (d_ext [T, Ng], d_x0, d_v0 [N]).  An environment's inputs depend on its index alone, so
environment k of a batch can be stepped in a handle of its own.  `salt` is 0; it is what changes if a draw ever violates the
node-distance condition of test_grad_edges_cpu.py (the threshold does not)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import hp_adjoint as ha
import hp_phase as hp
import hp_tangent as ht
import hp_tangent_kl as htk
import hp_tape_kl as hk

CEILING = 1e-9                # the project's ceiling on any float64 parity bound (test_gpu_adjoint.py: PARITY_BOUND)
FLOOR_BOUND = 1e-12           # the references against each other: about 30 x the 3e-14 / 4e-14 they show at Ng = 2722
NODE_DISTANCE = 1e-9          # cells: no reference position closer to a node than this, unless it sits on it by construction
MARGIN = 100.0                # two float64 evaluations summing in different orders (FFT / two scans, floating / fixed point)
KL_BINS = 16


@dataclass
class Case:
    id: str
    E: int
    N: int
    Ng: int
    L: float
    n0: float
    dt: float
    T: int
    every: int = 0            # the tape's checkpoint interval (0: the default, about sqrt(T))
    schedules: tuple = (0, 2)  # blocks_per_env: 0 = the planner's choice (resident at these sizes), > 0 = streaming
    salt: int = 0
    floor: dict = field(default_factory=dict)   # name -> reference-against-reference error (filled by `floors`)

    @property
    def ref_envs(self):
        """The environments the references are evaluated on: all of them, or for case H environments 0, E - 1 and three seeded
        others."""
        if self.E <= 8:
            return tuple(range(self.E))
        mid = np.random.default_rng([self.N, self.Ng, self.salt]).choice(np.arange(1, self.E - 1), 3, replace=False)
        return (0,) + tuple(int(e) for e in np.sort(mid)) + (self.E - 1,)

    @property
    def vrange(self):
        return -0.12 * self.L, 0.12 * self.L

    def setup(self, dt=None):
        return ha.Setup(self.N, self.Ng, self.L, self.n0, self.dt if dt is None else dt)

    def grid(self):
        return hp.Grid(KL_BINS, KL_BINS, self.L, *self.vrange, self.N, self.n0)


CASES = {c.id: c for c in (
    Case("A", 2, 1, 4, 50.0, 1.0, 0.1, 3),                    # smallest handle; bitsN = 0; one active lane
    Case("B", 3, 63, 5, 50.0, 1.0, 0.1, 4),                   # less than a wave of particles; odd mesh shorter than a wave
    Case("C", 2, 257, 33, 7.7, 0.37, 0.05, 5, every=2),       # L, n0, dt off default; 256 + 1 particles; ragged last segment
    Case("D", 1, 1025, 2722, 50.0, 1.0, 0.1, 2),              # largest float64 mesh; most nodes empty
    Case("E", 2, 2049, 64, 64.0, 2.5, 0.2, 6),                # dx = 1 exactly; placed edge particles; 2048 + 1 particles
    Case("F", 2, 4097, 250, 1.0, 4.0, 0.02, 3),               # small box, dense plasma; dt under the CFL clamp 0.031
    # (dt = 0.04: the handle clamps dt to 2 / sqrt(N / L) = 0.0447 at this N, and no case may be silently clamped)
    Case("G", 1, 100001, 250, 50.0, 1.0, 0.04, 2, schedules=(3,)),  # many workgroups and a one-particle tail (streaming)
    Case("H", 300, 2100, 16, 10.0, 1.0, 0.1, 3, schedules=(0,)),    # more environments than CUs; the 2048 / E grid clamp
)}
KL_CASES = ("C", "E", "F")
MOMENTS_CASES = ("C", "F")


def rel(a, b):
    """The norm of the existing GPU tests of every surface (test_gpu_adjoint.py: _rel)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(np.ravel(a - b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def env_inputs(c, e):
    """The inputs of environment e of case c (see the module's docstring), a dict of arrays."""
    if c.id == "H" and e == c.E - 1:
        e = 0                                   # case H: the last environment is given the first one's inputs
    rng = np.random.default_rng([c.N, c.Ng, c.salt, e])
    N, Ng, T, L = c.N, c.Ng, c.T, c.L
    d = {"x": rng.uniform(0.0, L, N), "v": rng.normal(0.0, 0.03 * L, N), "ext": 0.05 * rng.standard_normal((T, Ng))}
    for name, shape in (("cot", (T, 3)), ("cx", N), ("cv", N), ("ckl", T), ("cmom", (T, 3, Ng)), ("d_ext", (T, Ng)), ("d_x0", N),
                        ("d_v0", N)):
        d[name] = rng.standard_normal(shape)
    if c.id == "E" and e == 0:
        d["x"][:16] = 4.0 * np.arange(16)       # on nodes, at rest
        d["v"][:16] = 0.0
        d["x"][16], d["v"][16] = np.nextafter(L, 0.0), 0.0      # the last cell's right node folds to node 0
        d["x"][17], d["v"][17] = 0.0, -1.0      # wraps in the first drift
    return d


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """The batch of a case: name -> array with the environment axis where the device wants it (x, v, cx, cv, d_x0, d_v0
    [E, N]; ext, d_ext [T, E, Ng]; cot [T, 3, E]; ckl [T, E]; cmom [T, E, 3, Ng]) and feq [16, 16], shared."""
    c = CASES[cid]
    per = [env_inputs(c, e) for e in range(c.E)]
    out = {k: np.stack([p[k] for p in per]) for k in ("x", "v", "cx", "cv", "d_x0", "d_v0")}
    for k in ("ext", "d_ext", "ckl", "cmom"):
        out[k] = np.ascontiguousarray(np.stack([p[k] for p in per], axis=1))
    out["cot"] = np.ascontiguousarray(np.stack([p["cot"] for p in per], axis=2))
    lo, hi = c.vrange
    out["feq"] = np.random.default_rng([c.N, c.Ng, c.salt, 1 << 20]).uniform(0.1, 2.0, (KL_BINS, KL_BINS)) / (c.L * (hi - lo))
    return out


def directions(cid, e):
    """The K = 3 tangent directions of environment e: d_ext alone, d_x0 alone, d_v0 with d_ext (keyword dicts of the references)."""
    i = inputs(cid)
    return (dict(d_ext=i["d_ext"][:, e]), dict(d_x0=i["d_x0"][e]), dict(d_v0=i["d_v0"][e], d_ext=i["d_ext"][:, e]))


def _args(cid, e):
    i = inputs(cid)
    return i["x"][e], i["v"][e], i["ext"][:, e]


# ---- the references, once per process and environment: never modified by a test ------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_adjoint(cid, e):
    """(g_ext, g_x0, g_v0) by autograd, cotangents on the three energy traces and the final x, v."""
    i = inputs(cid)
    return ha.autograd_vjp(*_args(cid, e), CASES[cid].setup(), i["cot"][:, :, e], i["cx"][e], i["cv"][e])


@functools.lru_cache(maxsize=None)
def ref_tangent(cid, e):
    """Per direction (d_hist [T, 3], dx_T, dv_T, dE_mesh [T, Ng]) by torch forward mode."""
    return tuple(ht.torch_jvp(*_args(cid, e), CASES[cid].setup(), **u) for u in directions(cid, e))


@functools.lru_cache(maxsize=None)
def ref_tape_kl(cid, e):
    """(trace [T], (g_ext, g_x0, g_v0)) with cotangents on the KL trace, the energies and the final x, v."""
    c, i = CASES[cid], inputs(cid)
    S, G = c.setup(), c.grid()
    trace = hk.kl_trace(*_args(cid, e), S, G, i["feq"])
    g = hk.autograd_vjp(*_args(cid, e), S, G, i["feq"], i["ckl"][:, e], i["cot"][:, :, e], i["cx"][e], i["cv"][e])
    return trace, g


@functools.lru_cache(maxsize=None)
def ref_tangent_kl(cid, e):
    """Per direction d_kl [T] by torch forward mode."""
    c, i = CASES[cid], inputs(cid)
    return tuple(htk.torch_jvp(*_args(cid, e), c.setup(), c.grid(), i["feq"], **u)[1] for u in directions(cid, e))


@functools.lru_cache(maxsize=None)
def floors(cid):
    """The floor of every comparison of a case: the hand-written equations of the references against automatic differentiation
    of the restatement, in `rel`, worst over the reference environments (and over the directions and outputs of a tangent).
    Stored in the case's `floor` field as well: "adjoint", "tangent", "tape_kl"."""
    c, i = CASES[cid], inputs(cid)
    S, G = c.setup(), c.grid()
    f = {"adjoint": 0.0, "tangent": 0.0, "tape_kl": 0.0}
    for e in c.ref_envs:
        a = _args(cid, e)
        hand = ha.hand_vjp(*a, S, i["cot"][:, :, e], i["cx"][e], i["cv"][e])
        f["adjoint"] = max(f["adjoint"], *(rel(h, r) for h, r in zip(hand, ref_adjoint(cid, e))))
        for u, want in zip(directions(cid, e), ref_tangent(cid, e)):
            f["tangent"] = max(f["tangent"], *(rel(h, r) for h, r in zip(ht.hand_jvp(*a, S, **u), want)))
        hand = hk.hand_vjp(*a, S, G, i["feq"], i["ckl"][:, e], i["cot"][:, :, e], i["cx"][e], i["cv"][e])
        f["tape_kl"] = max(f["tape_kl"], *(rel(h, r) for h, r in zip(hand, ref_tape_kl(cid, e)[1])))
    c.floor.update(f)
    return f


def bound(cid, surface_bound, floor_name):
    """max(the surface's own bound, 100 x the case's floor), and never above the ceiling."""
    b = max(surface_bound, MARGIN * floors(cid)[floor_name])
    assert b <= CEILING, (cid, floor_name, b)
    return b


def node_distances(cid, e):
    """Distance to the nearest node, in cells, of q_1..q_4 and x' of every step of the reference: [T, 5, N]."""
    c = CASES[cid]
    S = c.setup()
    x, v, ext = _args(cid, e)
    out = np.empty((c.T, 5, c.N))
    for t in range(c.T):
        qs, ps, _, xn, _ = ha._np_forward_step(x, v, ext[t], S)
        for k, q in enumerate(qs + [xn]):
            f = np.mod(q, S.L) / S.dx
            out[t, k] = np.abs(f - np.round(f))
        x, v = xn, ps[-1]
    return out
