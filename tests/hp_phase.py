"""Restatement of the smoothed phase-space density and its KL in float64 torch, for the tests: the device's
integer CIC weights and their sums, the KL of estimate_KL_divergence, the hand vector-Jacobian product (what phase_vjp_kernel
computes) and a straight-through version for autograd (the values of the integer deposit, the derivative of the unquantised
weights)."""
import torch


class Grid:
    """nx x nv bins on [0, L] x [vmin, vmax] for N particles per environment, with the constants the host computes."""

    def __init__(self, nx, nv, L, vmin, vmax, N, n0=1.0):
        self.nx, self.nv, self.N = int(nx), int(nv), int(N)
        self.L, self.vmin, self.vmax, self.n0 = float(L), float(vmin), float(vmax), float(n0)
        self.dx = self.L / self.nx
        self.dv = (self.vmax - self.vmin) / self.nv
        self.rdx, self.rdv = 1.0 / self.dx, 1.0 / self.dv
        self.norm = self.n0 / self.dx / self.dv / self.N
        bits = max(1, self.N.bit_length())              # N < 2^bits: N particles of 2^(62 - bits) units stay below 2^62
        s = 62 - bits
        self.abits, self.bbits = (s + 1) // 2, s // 2
        self.unit = 2.0 ** -s


def locate(x, v, G):
    """inside, bins i0, i1, j0, j1, fractions fx, fv and the v-slope mask of every particle (phase_locate)."""
    inside = (x >= 0) & (x <= G.L) & (v >= G.vmin) & (v <= G.vmax)
    xs = torch.where(inside, x, torch.zeros_like(x))
    vs = torch.where(inside, v, torch.full_like(v, G.vmin))
    u = xs * G.rdx - 0.5
    fu = torch.floor(u)
    fx = u - fu
    i0 = fu.to(torch.int64)
    i1 = i0 + 1
    i0 = torch.where(i0 < 0, i0 + G.nx, i0).clamp(0, G.nx - 1)
    i1 = torch.where(i1 >= G.nx, i1 - G.nx, i1).clamp(0, G.nx - 1)
    w = (vs - G.vmin) * G.rdv - 0.5
    fw = torch.floor(w)
    j = fw.to(torch.int64)
    low, high = w < 0, (w >= 0) & (j >= G.nv - 1)
    slope = ~(low | high)
    j0 = torch.where(low, torch.zeros_like(j), torch.where(high, torch.full_like(j, G.nv - 1), j))
    j1 = torch.where(slope, j0 + 1, j0)
    fv = torch.where(slope, w - fw, torch.zeros_like(w))
    return inside, i0, i1, j0, j1, fx, fv, slope


def counts(x, v, G):
    """The integer sums [E, nx, nv] of the deposit (x, v: [E, N])."""
    inside, i0, i1, j0, j1, fx, fv, _ = locate(x, v, G)
    ua, ub = 1 << G.abits, 1 << G.bbits
    ax = torch.round(fx * float(ua)).to(torch.int64)
    av = torch.round(fv * float(ub)).to(torch.int64)
    E = x.shape[0]
    off = (torch.arange(E, dtype=torch.int64) * (G.nx * G.nv))[:, None]
    acc = torch.zeros(E * G.nx * G.nv, dtype=torch.int64)
    for i, wx in ((i0, ua - ax), (i1, ax)):
        for j, wv in ((j0, ub - av), (j1, av)):
            w = torch.where(inside, wx * wv, torch.zeros_like(wx))
            acc.index_add_(0, (off + i * G.nv + j).reshape(-1), w.reshape(-1))
    return acc.reshape(E, G.nx, G.nv)


def density(x, v, G):
    """f~ [E, nx, nv] with the device's values: ((double) sum * unit) * norm."""
    return (counts(x, v, G).to(torch.float64) * G.unit) * G.norm


def density_smooth(x, v, G):
    """f~ of the unquantised weights, differentiable in x and v (bins fixed, the CIC slopes inside them)."""
    inside, i0, i1, j0, j1, fx0, fv0, slope = locate(x.detach(), v.detach(), G)
    fx = x * G.rdx - 0.5 - torch.floor(x.detach() * G.rdx - 0.5)
    fv = torch.where(slope, (v - G.vmin) * G.rdv - 0.5 - torch.floor((v.detach() - G.vmin) * G.rdv - 0.5), v * 0.0)
    E = x.shape[0]
    off = (torch.arange(E, dtype=torch.int64) * (G.nx * G.nv))[:, None]
    f = torch.zeros(E * G.nx * G.nv, dtype=torch.float64)
    m = inside.to(torch.float64)
    for i, wx in ((i0, 1.0 - fx), (i1, fx)):
        for j, wv in ((j0, 1.0 - fv), (j1, fv)):
            f = f.index_add(0, (off + i * G.nv + j).reshape(-1), (m * wx * wv).reshape(-1))
    return (f * G.norm).reshape(E, G.nx, G.nv)


def density_st(x, v, G):
    """Straight-through: the device's values, the derivative of the unquantised weights."""
    fs = density_smooth(x, v, G)
    return density(x.detach(), v.detach(), G) + (fs - fs.detach())


def kl(f, feq, G):
    """sum rel_entr(f, feq + 1e-12) dx dv per environment [E] (feq [nx, nv] or [E, nx, nv])."""
    y = feq + 1e-12
    pos = f > 0
    r = torch.log(torch.where(pos, f, torch.ones_like(f)) / y)
    return torch.where(pos, f * r, torch.zeros_like(f)).sum(dim=(-2, -1)) * (G.dx * G.dv)


def vjp(x, v, feq, d_kl, G):
    """The hand vector-Jacobian product of d_kl . kl(f~(x, v)) -> (g_x, g_v) [E, N]: the cotangent grid of the finishing kernel
    gathered with the CIC slopes, as phase_vjp_kernel computes it."""
    f = density(x, v, G)
    y = feq + 1e-12
    pos = f > 0
    r = torch.log(torch.where(pos, f, torch.ones_like(f)) / y)
    g = torch.where(pos, d_kl[:, None, None] * ((r + 1.0) * (G.dx * G.dv)), torch.zeros_like(f))
    inside, i0, i1, j0, j1, fx, fv, slope = locate(x, v, G)
    gf = g.reshape(g.shape[0], -1)

    def at(i, j):
        return torch.gather(gf, 1, i * G.nv + j)
    g00, g01, g10, g11 = at(i0, j0), at(i0, j1), at(i1, j0), at(i1, j1)
    gx = (G.norm * G.rdx) * ((g10 - g00) * (1.0 - fv) + (g11 - g01) * fv)
    gv = (G.norm * G.rdv) * ((g01 - g00) * (1.0 - fx) + (g11 - g10) * fx)
    zero = torch.zeros_like(gx)
    return torch.where(inside, gx, zero), torch.where(inside & slope, gv, zero)


def autograd_vjp(x, v, feq, d_kl, G):
    """The same by autograd through density_st."""
    x = torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True)
    v = torch.as_tensor(v, dtype=torch.float64).clone().requires_grad_(True)
    J = (d_kl * kl(density_st(x, v, G), feq, G)).sum()
    gx, gv = torch.autograd.grad(J, (x, v))
    return gx, gv
