"""What the device checkpointers share: the library and the device as Driver takes them, and a variable -- a Quantity (a
transpose view, a 2-D field, a float32 field), a tensor or a numpy array -- described to the kernels as a base pointer,
extents (ni, nj, nk) in STORAGE order and strides (1, sj, sk)."""
import numpy as np
import torch

from ... import _launch, _lib


class DeviceSide:
    def __init__(self, lib=None, device=None):
        """lib: the kernel library (default: the product library, loaded at the first call); device: where uploaded arrays and
        the accumulators live (default: the current device; "cpu" with the emulation test library)."""
        self._lib = lib
        self._device = torch.device(device) if device is not None else None

    @property
    def lib(self):
        if self._lib is None:
            self._lib = _lib.load()
        return self._lib

    @property
    def device(self):
        if self._device is None:
            self._device = _launch.default_device(self.lib)
        return self._device

    @property
    def real(self):
        return _launch.real_of(self.lib)

    def stream(self):
        return _launch.stream_of(self.device)

    def describe(self, name, array):
        """A Variable for what a checkpoint call handed over.  numpy arrays are uploaded (as the library's storage type);
        a tensor is copied only if its smallest stride is not 1 or its rows overlap."""
        t = array.data if hasattr(array, "dims") else array
        if not torch.is_tensor(t):
            t = np.asarray(t)
            if not np.issubdtype(t.dtype, np.floating):  # (as an integer tensor below: no silent conversion)
                raise TypeError(f"{name}: a checkpointed variable holds floats, not {t.dtype}")
            t = torch.as_tensor(np.ascontiguousarray(np.asarray(t)), dtype=self.real, device=self.device)
        if t.dtype != self.real:
            if not t.dtype.is_floating_point:
                raise TypeError(f"{name}: a checkpointed variable holds floats, not {t.dtype}")
            raise TypeError(f"{name}: dtype {t.dtype} does not match the library's storage type {self.real}")
        _launch.check_library(self.lib, t.device, name=name)
        if t.dim() < 1 or t.dim() > 3:
            raise ValueError(f"{name}: variables have one to three axes, not {t.dim()}")
        var = Variable.of(name, t)
        return var if var is not None else Variable.of(name, t.contiguous())


class Variable:
    """tensor: the array as handed over (its axes in the caller's order); perm[a]: the handed axis that is storage axis a
    (0: x, the fastest); extents / strides: in storage order, padded to three with extent 1."""

    def __init__(self, name, tensor, perm, extents, strides):
        self.name, self.tensor, self.perm, self.extents, self.strides = name, tensor, perm, extents, strides

    @classmethod
    def of(cls, name, t):
        """None if the tensor's memory is no (1, sj, sk) storage."""
        axes = [a for a in range(t.dim()) if t.shape[a] > 1]
        axes.sort(key=lambda a: t.stride(a))
        perm = axes + [a for a in range(t.dim()) if t.shape[a] <= 1]  # (axes of length 1 go last: their stride means nothing)
        if t.numel() == 0:
            raise ValueError(f"{name}: an empty variable")
        extents = [t.shape[a] for a in perm] + [1] * (3 - t.dim())
        strides = [t.stride(a) for a in axes]
        if strides and strides[0] != 1:
            return None
        ni, nj, _ = extents
        sj = strides[1] if len(strides) > 1 else ni
        sk = strides[2] if len(strides) > 2 else sj * nj
        if sj < ni or sk < sj * (nj - 1) + ni:
            return None
        return cls(name, t, tuple(perm), tuple(extents), (1, sj, sk))

    @property
    def count(self):
        return self.extents[0] * self.extents[1] * self.extents[2]

    def fill(self, item):
        item.field = self.tensor.data_ptr()
        item.ni, item.nj, item.nk = self.extents
        item.sj, item.sk = self.strides[1], self.strides[2]
