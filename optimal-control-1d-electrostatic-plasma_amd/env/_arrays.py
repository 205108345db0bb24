"""Where the arrays of one call of the differentiation layer live: host memory as NumPy arrays, or device memory
as float64 CUDA tensors.  `Mem` is decided once per call and is the only place that knows which; torch is imported only when a
call works on the device.  `directions` reads the number of directions of a forward-mode call off its inputs."""
import numpy as np

from .._abi import PIC_DEVICE, PIC_HOST


def directions(who, base, given, K=None, walk=None):
    """(K, batched) of a forward-mode call: the number of directions and whether its arrays carry a leading K axis.  `given`:
    name -> array (None = absent); `base`: name -> shape without K.  From K if given (then they do), else from the inputs;
    `walk`: the fixed (K, batched) of a walk in progress, which the inputs of a step must match.  ValueError(who: ...) if the
    inputs disagree or one has another shape.  K is not capped here: the library refuses K > 8."""
    shapes = {k: tuple(a.shape) for k, a in given.items() if a is not None}
    if walk is not None:
        K, batched = walk
    else:
        ks = {s[0] for k, s in shapes.items() if len(s) == len(base[k]) + 1}
        if K is not None:
            ks.add(int(K))
        if len(ks) > 1:
            raise ValueError(f"{who}: the inputs disagree on the number of directions: {sorted(ks)}")
        batched = bool(ks)
        K = ks.pop() if ks else 1
    for k, s in shapes.items():
        want = ((K,) if batched else ()) + base[k]
        if s != want:
            raise ValueError(f"{who}: {k} must have shape {want}, not {s}")
    return K, batched


class Mem:
    __slots__ = ("device_index", "on_device", "shared_stream", "kind")

    def __init__(self, device_index, on_device, shared_stream):
        self.device_index, self.on_device, self.shared_stream = device_index, bool(on_device), bool(shared_stream)
        self.kind = PIC_DEVICE if on_device else PIC_HOST

    @classmethod
    def of(cls, env, *arrays, force_device=False):
        """The memory of a call on `env` with these arguments (None allowed): the device if any of them is a CUDA tensor."""
        on_device = force_device or any(hasattr(a, "is_cuda") and a.is_cuda for a in arrays)
        return cls(env.device, on_device, env._torch_stream is not None)

    def f64(self, a, shape=None):
        """a (None stays None) as a C-contiguous float64 array in this memory, reshaped to `shape` if given."""
        if a is None:
            return None
        if self.on_device:
            import torch
            a = torch.as_tensor(a, dtype=torch.float64, device=f"cuda:{self.device_index}")
            return (a if shape is None else a.reshape(shape)).contiguous()
        a = np.asarray(a, dtype=np.float64)
        return np.ascontiguousarray(a if shape is None else a.reshape(shape))

    def empty(self, shape):
        if self.on_device:
            import torch
            return torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device_index}")
        return np.empty(shape)

    def zeros(self, shape):
        if self.on_device:
            import torch
            return torch.zeros(shape, dtype=torch.float64, device=f"cuda:{self.device_index}")
        return np.zeros(shape)

    def out(self, shape):
        """An output of a tape call: uninitialised on the device (a fill would be one more launch per output), zero-filled on
        the host, as the host bindings hand theirs to the library."""
        if self.on_device:
            import torch
            return torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device_index}")
        return np.zeros(shape)

    @staticmethod
    def addr(a):
        """The address of a: 0 for None or an empty tensor.  (The bare address keeps no reference: see _abi._ptr.)"""
        if a is None:
            return 0
        if hasattr(a, "data_ptr"):
            return a.data_ptr() if a.numel() else 0
        return a.__array_interface__["data"][0]

    def stack_energies(self, T, E, d_KE, d_PE, d_PE_reward):
        """The cotangents of the three energy traces as one [T, 3, E] array (each None = 0), None if all three are None."""
        if d_KE is None and d_PE is None and d_PE_reward is None:
            return None
        hist = self.zeros((T, 3, E))
        for k, a in enumerate((d_KE, d_PE, d_PE_reward)):
            if a is not None:
                hist[:, k] = self.f64(a, (T, E))
        return hist

    # Stream ordering of a call that works on device memory next to torch: on a stream shared with torch (use_torch_stream) the
    # stream alone orders it; otherwise torch's current stream is drained before the call (enter) and, where the caller hands
    # the outputs straight back to torch, the handle's own stream after it (leave).  Host memory: the library stages and waits.
    def enter(self):
        if self.on_device and not self.shared_stream:
            import torch
            torch.cuda.current_stream(self.device_index).synchronize()

    def leave(self, handle):
        if self.on_device and not self.shared_stream:
            handle.sync()
