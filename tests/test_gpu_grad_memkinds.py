"""Host memory against device memory in the Python differentiation layer: every entry of BatchedPIC that takes
NumPy arrays or CUDA tensors (backward, tangent, the walk, tape_kl, kl_smooth[_grad]) returns the same bits either way, on a handle
with its own stream and on torch's.  Both ways run the same kernels in the same order, so equality is the condition.

One shape with no two axes of equal length, so that a transposed or mis-stacked argument shows: 2 environments of N = 1000 (no
multiple of 256) on 64 nodes, max_mode = 2 (2M = 4), T = 5 steps with a checkpoint every 2 (the last segment is ragged), K = 2
tangent directions, 8 x 6 phase-space bins."""
import numpy as np
import pytest
import torch

from oracle import pic_oracle as po

pytestmark = pytest.mark.gpu

L = 50.0
E, N, NG, M, T, EVERY, K = 2, 1000, 64, 2, 5, 2, 2
NX, NV, VMIN, VMAX = 8, 6, -6.0, 6.0
STREAMS = ["own", "torch"]


def _make(stream):
    import ocplasma_amd as oc
    from ocplasma_amd.env.batched import BatchedPIC
    env = BatchedPIC(E, N, NG, L=L, dt=0.1)
    X, V = np.empty((E, N)), np.empty((E, N))
    for e in range(E):
        X[e], V[e] = po.synthetic_bump_on_tail(N, L, seed=3 + 7 * e)
    env.reset(X, V)
    env.set_actuator(oc.E_field(L, NG, M))
    if stream == "torch":
        env.use_torch_stream()
    return env


def _rng(seed):
    return np.random.default_rng(seed)


def _actions(seed=1):
    return _rng(seed).uniform(-0.5, 0.5, (T, E, 2 * M))


def _kl():
    return dict(feq=_rng(2).uniform(0.0, 2.0 / (L * (VMAX - VMIN)), (NX, NV)), vmin=VMIN, vmax=VMAX)


def _cuda(a):
    return None if a is None else torch.as_tensor(a, device="cuda")


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _assert_same(host, dev, what):
    """host: NumPy arrays from NumPy arguments; dev: CUDA tensors from CUDA arguments; equal bit for bit."""
    assert isinstance(host, np.ndarray) and host.dtype == np.float64, (what, type(host))
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64, (what, type(dev))
    assert host.shape == tuple(dev.shape), (what, host.shape, tuple(dev.shape))
    assert np.array_equal(host, _host(dev)), what


def _assert_same_dict(host, dev, keys):
    assert list(host) == list(dev) == keys, (list(host), list(dev))
    for k in keys:
        _assert_same(host[k], dev[k], k)


def _both(fn, **kw):
    """fn with NumPy arguments, then with the same values as CUDA tensors."""
    return fn(**kw), fn(**{k: _cuda(a) for k, a in kw.items()})


@pytest.mark.parametrize("stream", STREAMS)
def test_backward_of_an_action_tape(stream):
    """(a), and the raw binding: BatchedPIC.backward adds nothing to pic_tape_backward."""
    env, r = _make(stream), _rng(10)
    env.start_tape(T, EVERY)
    env.step_actions_traj(_actions())
    cot = dict(d_KE=r.standard_normal((T, E)), d_PE_reward=r.standard_normal((T, E)), d_x=r.standard_normal((E, N)),
               d_v=np.asfortranarray(r.standard_normal((E, N))))
    host, dev = _both(env.backward, **cot)
    _assert_same_dict(host, dev, ["ext", "x0", "v0", "actions"])
    assert host["ext"].shape == (T, E, NG) and host["actions"].shape == (T, E, 2 * M) and host["x0"].shape == (E, N)
    # the library itself, reached through ctypes alone
    hist = np.zeros((T, 3, E))
    hist[:, 0], hist[:, 2] = cot["d_KE"], cot["d_PE_reward"]
    cx, cv = np.ascontiguousarray(cot["d_x"]), np.ascontiguousarray(cot["d_v"])
    raw = {"ext": np.zeros((T, E, NG)), "actions": np.zeros((T, E, 2 * M)), "x0": np.zeros((E, N)), "v0": np.zeros((E, N))}
    rc = env._h.lib.pic_tape_backward(env._h._h, hist.ctypes.data, cx.ctypes.data, cv.ctypes.data, 0, raw["ext"].ctypes.data,
                                      raw["actions"].ctypes.data, raw["x0"].ctypes.data, raw["v0"].ctypes.data)
    assert rc == 0
    bound = env._h.tape_backward(hist, cx, cv, ext=True, actions=True, particles=True)
    assert sorted(bound) == ["g_actions", "g_ext", "g_v0", "g_x0"]
    for k in ("ext", "actions", "x0", "v0"):
        assert np.array_equal(host[k], raw[k]), k
        assert np.array_equal(host[k], bound["g_" + k]), k
    assert np.any(host["ext"]) and np.any(host["x0"])
    env.stop_tape()
    env.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_backward_of_a_gain_law_tape(stream):
    """(b)"""
    env, r = _make(stream), _rng(11)
    G = np.stack([np.diag([-1.0] * M + [1.0] * M)] * E) + 0.1 * r.standard_normal((E, 2 * M, 2 * M))
    env.start_tape(T, EVERY)
    env.step_feedback_gain(G, T)
    cot = dict(d_KE=r.standard_normal((T, E)), d_PE_reward=r.standard_normal((T, E)), d_x=r.standard_normal((E, N)),
               d_v=r.standard_normal((E, N)), d_modes=r.standard_normal((T, E, 2 * M)))
    host, dev = _both(env.backward, **cot)
    _assert_same_dict(host, dev, ["ext", "x0", "v0", "actions", "modes", "gain"])
    assert host["gain"].shape == (E, 2 * M, 2 * M) and host["modes"].shape == (T, E, 2 * M) and np.any(host["gain"])
    env.stop_tape()
    env.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_backward_and_trace_of_a_kl_tape(stream):
    """(c)"""
    env, r = _make(stream), _rng(12)
    env.start_tape(T, EVERY, kl=_kl())
    env.step_actions_traj(_actions())
    trace = env.tape_kl()
    assert trace.shape == (T, E)
    _assert_same(trace, env.tape_kl(on_device=True), "tape_kl")
    cot = dict(d_KL=r.standard_normal((T, E)), d_PE_reward=r.standard_normal((T, E)))
    host, dev = _both(env.backward, **cot)
    _assert_same_dict(host, dev, ["ext", "x0", "v0", "actions"])
    plain = env.backward(d_PE_reward=cot["d_PE_reward"])              # (d_KL = None clears the rows: the KL's part is gone)
    assert not np.array_equal(plain["ext"], host["ext"])
    env.stop_tape()
    env.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_tangent(stream):
    """(d)"""
    env, r = _make(stream), _rng(13)
    env.start_tape(T, EVERY)
    env.step_actions_traj(_actions())
    keys = ["KE", "PE", "PE_reward", "x", "v", "E_mesh"]
    tan = dict(d_actions=r.standard_normal((K, T, E, 2 * M)), d_x0=r.standard_normal((K, E, N)), d_v0=r.standard_normal((K, E, N)))
    host, dev = _both(lambda **kw: env.tangent(fields=True, **kw), **tan)
    _assert_same_dict(host, dev, keys)
    assert host["KE"].shape == (K, T, E) and host["x"].shape == (K, E, N) and host["E_mesh"].shape == (K, T, E, NG)
    one, one_dev = _both(lambda **kw: env.tangent(fields=True, **kw), **{k: a[1] for k, a in tan.items()})
    _assert_same_dict(one, one_dev, keys)
    assert one["KE"].shape == (T, E) and one["x"].shape == (E, N) and one["E_mesh"].shape == (T, E, NG)
    env.stop_tape()
    env.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_walk(stream):
    """(e)"""
    env, r = _make(stream), _rng(14)
    env.start_tape(T, EVERY, kl=_kl())
    env.step_actions_traj(_actions())
    steps = [dict(d_energies=r.standard_normal((3, E)), d_modes=r.standard_normal((E, 2 * M)), d_kl=r.standard_normal(E))
             for _ in range(T)]
    d_x0 = r.standard_normal((E, N))

    def walk(conv):
        w = env.walk()
        out = [w.step(**{k: conv(a) for k, a in s.items()}) for s in steps]
        return out, w.end(d_x0=conv(d_x0))
    (hs, he), (ds, de) = walk(lambda a: a), walk(_cuda)
    for i, ((th, gh, ah), (td, gd, ad)) in enumerate(zip(hs, ds)):
        assert th == td == T - 1 - i
        _assert_same(gh, gd, f"g_ext[{th}]")
        _assert_same(ah, ad, f"g_actions[{th}]")
        assert gh.shape == (E, NG) and ah.shape == (E, 2 * M)
    for k, h, d in zip(("g_x0", "g_v0"), he, de):
        _assert_same(h, d, k)
        assert h.shape == (E, N) and np.any(h)
    env.stop_tape()
    env.close()


@pytest.mark.parametrize("stream", STREAMS)
def test_kl_smooth_and_its_gradient(stream):
    """(f)"""
    env, kl = _make(stream), _kl()
    env.step_actions_traj(_actions()[:2])
    feq, d_kl = kl["feq"], _rng(15).standard_normal(E)
    _assert_same(env.kl_smooth(feq, VMIN, VMAX), env.kl_smooth(_cuda(feq), VMIN, VMAX), "kl_smooth")
    host, dev = _both(lambda **kw: env.kl_smooth_grad(vmin=VMIN, vmax=VMAX, **kw), feq=feq, d_kl=d_kl)
    for k, h, d in zip(("g_x", "g_v"), host, dev):
        _assert_same(h, d, k)
        assert h.shape == (E, N) and np.any(h)
    env.close()
