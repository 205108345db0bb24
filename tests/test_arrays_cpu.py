"""The host half of env._arrays.Mem: the one place that decides between host and device memory for a call of the
differentiation layer.  No library and no GPU."""
import numpy as np
import torch

import ocplasma_amd  # noqa: F401
from ocplasma_amd._abi import PIC_HOST
from ocplasma_amd.env._arrays import Mem


class _Env:
    device, _torch_stream = 0, None


class _NoSync:
    def sync(self):
        raise AssertionError("a call in host memory must not synchronise the handle")


def test_f64_gives_c_contiguous_float64_of_the_shape():
    mem = Mem(0, False, False)
    a = np.asfortranarray(np.arange(24, dtype=np.float32).reshape(4, 6))
    b = mem.f64(a, (2, 2, 6))
    assert b.dtype == np.float64 and b.flags.c_contiguous and b.shape == (2, 2, 6)
    assert np.array_equal(b.reshape(4, 6), a)
    c = mem.f64(a)
    assert c.dtype == np.float64 and c.flags.c_contiguous and c.shape == (4, 6) and np.array_equal(c, a)
    assert mem.f64(None) is None and mem.f64(None, (3,)) is None


def test_stack_energies():
    mem, T, E = Mem(0, False, False), 5, 2
    assert mem.stack_energies(T, E, None, None, None) is None
    pe = np.arange(1.0, 1.0 + T * E).reshape(T, E)
    h = mem.stack_energies(T, E, None, pe, None)
    assert h.shape == (T, 3, E) and h.dtype == np.float64 and h.flags.c_contiguous
    assert np.array_equal(h[:, 1], pe) and not h[:, 0].any() and not h[:, 2].any()
    h = mem.stack_energies(T, E, torch.as_tensor(pe), None, pe.ravel().astype(np.float32))
    assert np.array_equal(h[:, 0], pe) and not h[:, 1].any() and np.array_equal(h[:, 2], pe)


def test_addr():
    a = np.zeros((3, 4))
    assert Mem.addr(None) == 0
    assert Mem.addr(a) == a.ctypes.data
    assert Mem.addr(a[1:]) == a[1:].ctypes.data == a.ctypes.data + 4 * 8


def test_outputs_on_the_host():
    mem = Mem(0, False, False)
    for make in (mem.empty, mem.zeros, mem.out):
        a = make((2, 3))
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (2, 3) and a.flags.c_contiguous
    assert not mem.zeros((2, 3)).any() and not mem.out((2, 3)).any()


def test_numpy_and_cpu_tensors_are_host_memory():
    mem = Mem.of(_Env(), np.zeros(3), None, torch.zeros(3, dtype=torch.float64), [1.0, 2.0])
    assert not mem.on_device and mem.kind == PIC_HOST
    assert not Mem.of(_Env()).on_device
    assert Mem.of(_Env(), force_device=True).on_device


def test_stream_ordering_touches_nothing_on_the_host(monkeypatch):
    def no_stream(*a, **k):
        raise AssertionError("a call in host memory must not touch torch's stream")
    monkeypatch.setattr(torch.cuda, "current_stream", no_stream)
    for shared in (False, True):
        mem = Mem(0, False, shared)
        mem.enter()
        mem.leave(_NoSync())
