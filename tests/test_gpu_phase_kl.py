"""The smoothed phase-space density and its KL on the device (pic_phase_kl_smooth*): against the float64 torch
restatement (tests/hp_phase.py), against the histogram KL where the two must coincide, bitwise independence of the launch
geometry, the schedule and the batch, and the contract.

Bounds are 100x what was measured on an MI355X (reported through conftest's record_measure under keys "phase_kl.*")."""
import numpy as np
import pytest
import torch

import hp_phase as hp
from conftest import record_measure
from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
VMIN, VMAX = -6.0, 6.0
# measured: f~ bitwise equal to the restatement (its integer weights are the device's), KL 3.4e-16, gradient 5.4e-16 relative
# (the issue's ceilings: 1e-14, 1e-12, 1e-9)
TOL_KL, TOL_GRAD = 3.4e-14, 5.4e-14


def _make(E, N, Ng=64, seed=1, steps=2, **kw):
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, Ng, L=L, dt=0.1, **kw)
    X, V = np.empty((E, N)), np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=seed + 7 * e)
    env.reset(X, V)
    if steps:
        env.step(nsteps=steps)
    return env


def _grid(env, nx, nv, vmin=VMIN, vmax=VMAX):
    return hp.Grid(nx, nv, env.L, vmin, vmax, env.N, env.n0)


def _target(E, nx, nv, per_env, seed):
    rng = np.random.default_rng(seed)
    shape = (E, nx, nv) if per_env else (nx, nv)
    return rng.uniform(0.0, 2.0 / (L * (VMAX - VMIN)), shape)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("nx,nv", [(32, 32), (250, 250), (1024, 64)])
def test_density_and_kl_match_the_restatement(nx, nv):
    env = _make(3, 3000)
    x, v = (torch.as_tensor(a) for a in env.particles())
    G = _grid(env, nx, nv)
    f_dev = env.phase_density_smooth((nx, nv), VMIN, VMAX)
    f_ref = hp.density(x, v, G).numpy()
    record_measure(f"phase_kl.f_{nx}x{nv}", _rel(f_dev, f_ref))
    assert np.array_equal(f_dev, f_ref)
    for per_env in (False, True):
        feq = _target(3, nx, nv, per_env, seed=nx)
        kl_dev = env.kl_smooth(feq, VMIN, VMAX)
        kl_ref = hp.kl(hp.density(x, v, G), torch.as_tensor(feq), G).numpy()
        ek = _rel(kl_dev, kl_ref)
        record_measure(f"phase_kl.kl_{nx}x{nv}_{'env' if per_env else 'shared'}", ek)
        assert ek <= TOL_KL
    env.close()


def test_mass_and_bin_centres_agree_with_the_histogram():
    env = _make(2, 4000)
    x, v = (torch.as_tensor(a) for a in env.particles())
    G = _grid(env, 40, 40)
    f = env.phase_density_smooth(40, VMIN, VMAX)
    assert np.array_equal(f, hp.density(x, v, G).numpy())          # the device's integer sums are the restatement's ...
    counts = env._h.phase_histogram(40, VMIN, VMAX).astype(np.int64)
    unit = 1 << (G.abits + G.bbits)
    assert np.array_equal(hp.counts(x, v, G).sum(dim=(1, 2)).numpy(), counts.sum(axis=(1, 2)) * unit)   # ... whose mass is exact
    env.close()
    # power-of-two bin widths, particles on the bin centres: f~ is estimate_f's f and KL~ is pic_phase_kl's KL
    from ocplasma_amd.env.batched import BatchedPIC
    Lc, nb, N, E = 64.0, 32, 2048, 2
    env = BatchedPIC(E, N, 64, L=Lc, dt=0.1)
    rng = np.random.default_rng(4)
    i, j = rng.integers(0, nb, (E, N)), rng.integers(0, nb, (E, N))
    env.reset((i + 0.5) * (Lc / nb), -16.0 + (j + 0.5) * (32.0 / nb))
    f_smooth = env.phase_density_smooth(nb, -16.0, 16.0)
    f_hist = env.phase_density(nb, -16.0, 16.0)
    assert np.array_equal(f_smooth, f_hist)
    feq = rng.uniform(0.0, 2e-3, (nb, nb))
    assert _rel(env.kl_smooth(feq, -16.0, 16.0), env.kl_divergence(feq, -16.0, 16.0)) <= 1e-13
    env.close()


def test_gradient_matches_autograd_of_the_restatement():
    env = _make(2, 3000)
    x, v = (torch.as_tensor(a) for a in env.particles())
    for nx, nv, per_env in ((32, 32, False), (250, 250, True)):
        G = _grid(env, nx, nv)
        feq = _target(2, nx, nv, per_env, seed=3)
        d = np.array([0.7, 1.3])
        gx, gv = env.kl_smooth_grad(feq, d, VMIN, VMAX)
        ax, av = hp.autograd_vjp(x, v, torch.as_tensor(feq), torch.as_tensor(d), G)
        scale = max(float(ax.abs().max()), float(av.abs().max()))
        err = max(float(np.abs(gx - ax.numpy()).max()), float(np.abs(gv - av.numpy()).max())) / scale
        record_measure(f"phase_kl.grad_{nx}x{nv}", err)
        assert err <= TOL_GRAD
        # CUDA tensors in, CUDA tensors out, the same bits
        tx, tv = env.kl_smooth_grad(torch.as_tensor(feq, device="cuda"), torch.as_tensor(d, device="cuda"), VMIN, VMAX)
        assert tx.is_cuda and np.array_equal(tx.cpu().numpy(), gx) and np.array_equal(tv.cpu().numpy(), gv)
        kt = env.kl_smooth(torch.as_tensor(feq, device="cuda"), VMIN, VMAX)
        assert kt.is_cuda and np.array_equal(kt.cpu().numpy(), env.kl_smooth(feq, VMIN, VMAX))
    env.close()


def _all(env, feq):
    return (env.phase_density_smooth(feq.shape[-2:], VMIN, VMAX), env.kl_smooth(feq, VMIN, VMAX),
            *env.kl_smooth_grad(feq, None, VMIN, VMAX))


def test_multi_workgroup_deposit_is_exact_and_independent_of_the_batch():
    """N = 100001 (odd: the last 16-byte tile holds one particle) on a 250 x 250 grid (8 bands): one environment deposits with 13
    workgroups per band, six with 11 (phase_args: about 512 workgroups in all, at least 8192 particles each), so the particle
    ranges start and end at different places and several workgroups flush into the same bins.  Environment 3 of the six holds
    the particles of the single one: every output of it must be the same bits, and the restatement's."""
    from ocplasma_amd.env.batched import BatchedPIC
    N, nb = 100001, 250
    feq = _target(1, nb, nb, False, seed=5)
    X, V = po.synthetic_bump_on_tail(N, L, seed=21)
    outs = []
    for E, k in ((1, 0), (6, 3)):
        env = BatchedPIC(E, N, 128, L=L, dt=0.1)
        Xs, Vs = np.empty((E, N)), np.empty((E, N))
        for e in range(E):
            Xs[e], Vs[e] = (X, V) if e == k else po.synthetic_bump_on_tail(N, L, seed=30 + e)
        env.reset(Xs, Vs)
        outs.append([a[k] for a in _all(env, feq)])
        if E == 1:
            x, v = (torch.as_tensor(a) for a in env.particles())
        env.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    G = hp.Grid(nb, nb, L, VMIN, VMAX, N)
    f, kl, gx, gv = outs[0]
    assert np.array_equal(f, hp.density(x, v, G)[0].numpy())
    assert _rel(kl, hp.kl(hp.density(x, v, G), torch.as_tensor(feq), G).numpy()[0]) <= TOL_KL
    ax, av = hp.autograd_vjp(x, v, torch.as_tensor(feq), torch.ones(1, dtype=torch.float64), G)
    scale = max(float(ax.abs().max()), float(av.abs().max()))
    err = max(float(np.abs(gx - ax[0].numpy()).max()), float(np.abs(gv - av[0].numpy()).max())) / scale
    record_measure("phase_kl.grad_multi_workgroup", err)
    assert err <= TOL_GRAD


def test_bitwise_independent_of_the_schedule_that_stepped_the_state():
    """The same environments stepped by the resident kernel and by streaming sweeps (their particles are the same bits) give the
    same bits here too; the phase kernels read only the stored particles."""
    feq = _target(3, 32, 32, False, seed=9)
    outs = []
    for kw in ({}, {"blocks_per_env": 2}):                          # N = 5000: resident by default, then streaming
        env = _make(3, 5000, Ng=128, steps=3, **kw)
        assert env._h.schedule() == ("resident" if not kw else "streaming")
        outs.append(_all(env, feq))
        env.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_contract_refusals():
    import ocplasma_amd as oc
    env = _make(1, 2000, steps=0)
    feq = np.ones((8, 8))
    for bins in (0, 1025, (8, 0), (1025, 8)):
        with pytest.raises(oc._abi.PicError, match="pic_phase_kl_smooth"):
            env.phase_density_smooth(bins, VMIN, VMAX)
    with pytest.raises(oc._abi.PicError, match="vmin < vmax"):
        env.kl_smooth(feq, 1.0, 1.0)
    with pytest.raises(oc._abi.PicError, match="vmin < vmax"):
        env.kl_smooth_grad(feq, None, 1.0, -1.0)
    with pytest.raises(ValueError, match="feq"):
        env.kl_smooth(np.ones((2, 8, 8)), VMIN, VMAX)
    env.close()
    from ocplasma_amd.env.batched import BatchedPIC
    env32 = BatchedPIC(1, 2000, 64, L=L, dt=0.1, dtype="float32")
    env32.reset_sampled(seed=1)
    with pytest.raises(oc._abi.PicError, match="float64"):
        env32.kl_smooth(feq, VMIN, VMAX)
    env32.close()
