"""What the host side of every entry-point call shares: the stream handed to the entry point, whether a library goes with the
tensors, the storage geometry of the fields of a call, a window of a field as a table item, staging buffers and their copies.

The rules: a stream is always asked for BY DEVICE -- the device the call's tensors live on, never "the current one"; there is
one derivation of ``_lib.Geom`` from strides (``geometry``; ``util.grid.geom_struct`` and the halo updaters' specs know theirs
without looking at a tensor); and one mapping of a quantity, a level of it or an explicit box to the eight integers of an item
(``window_of`` / ``set_window``).  Plain functions; this module imports nothing of the package but ``_lib``.
"""
import ctypes as C

import torch

from . import _lib


# ---- the stream ---------------------------------------------------------------------------------------------------------------
def stream_of(device):
    """The current stream of `device` as an entry point takes it; None for the CPU (the emulation library)."""
    if torch.device(device).type == "cpu":
        return None
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def wait_for(device):
    """Wait until the current stream of `device` has run what was launched on it; nothing to wait for on the CPU."""
    if torch.device(device).type != "cpu":
        torch.cuda.current_stream(device).synchronize()


# ---- the library against the tensors --------------------------------------------------------------------------------------------
def is_emulation(lib) -> bool:
    return "emulation" in lib.version()


def default_device(lib) -> torch.device:
    """Where a library's fields live when nobody says: the CPU for the emulation test library, else the current device."""
    return torch.device("cpu") if is_emulation(lib) else torch.device("cuda", torch.cuda.current_device())


def real_of(lib) -> torch.dtype:
    """The library's storage type."""
    return torch.float32 if lib.real_bytes == 4 else torch.float64


def check_library(lib, device, dtype=None, name=None):
    """Raise unless `lib` stores `dtype`, where given (ValueError), and runs on tensors on `device` (PaceError)."""
    prefix = "" if name is None else f"{name}: "
    if dtype is not None and dtype != real_of(lib):
        raise ValueError(f"{prefix}field dtype {dtype} does not match the library's storage type {real_of(lib)}")
    if (torch.device(device).type == "cpu") != is_emulation(lib):
        raise _lib.PaceError(f"{prefix}CPU tensors go with the emulation test library, device tensors with the product library")


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def geometry(fields, refuse, differ, ndim=(2, 3), fewer_levels=False):
    """The one storage geometry of the fields (Quantities, gather Windows or tensors) of a call, from their strides.

    Every field has `ndim` axes and stride 1 along the first, or ValueError(refuse(field)).  All share (n, sj), and the 3-D ones
    (nk, sk), or ValueError(differ); with `fewer_levels` the first 3-D field gives nk and a later one may have fewer levels, not
    more.  Without a 3-D field nk = 1 and sk = sj * (n + 7): a plane item reads neither, the entry points want one level."""
    layouts = []  # (shape, strides) per field: each asked of torch once, this runs at every call
    for f in fields:
        t = f if isinstance(f, torch.Tensor) else f.data
        layouts.append((t.shape, t.stride()))
        if len(t.shape) not in ndim or layouts[-1][1][0] != 1:
            raise ValueError(refuse(f))
    n, sj = layouts[0][0][0] - 7, layouts[0][1][1]
    volumes = [(shape[2] - 1, stride[2]) for shape, stride in layouts if len(shape) == 3]
    nk, sk = volumes[0] if volumes else (1, sj * (n + 7))
    if any((shape[0] - 7, stride[1]) != (n, sj) for shape, stride in layouts):
        raise ValueError(differ)
    if any(k != sk or (levels > nk if fewer_levels else levels != nk) for levels, k in volumes):
        raise ValueError(differ)
    return _lib.Geom(n, nk, sj, 0, sk)


# ---- windows --------------------------------------------------------------------------------------------------------------------
def window_of(quantity, level=None, window=None):
    """(pointer, kind, i0, j0, k0, ni, nj, nk) of an item: the compute domain of a 3-D quantity is a WINDOW3D; a 2-D quantity is
    a PLANE; `level` of a 3-D quantity is a PLANE whose pointer is that level's.  `window` replaces the compute domain by an
    explicit (i0, j0, k0, ni, nj, nk) of the storage (a PLANE has k0 = 0 and nk = 1)."""
    data = quantity.data
    volume = level is None and data.dim() == 3
    if window is None:
        o, e = quantity.origin, quantity.extent
        window = (o[0], o[1], o[2], e[0], e[1], e[2]) if volume else (o[0], o[1], 0, e[0], e[1], 1)
    pointer = quantity.ptr + (level * data.stride(2) * data.element_size() if level else 0)
    return (pointer, _lib.DIAG_WINDOW3D if volume else _lib.DIAG_PLANE) + tuple(window)


def set_window(item, window):
    """What window_of returned into a DiagItem, UnpackItem, CubeItem, RestartItem or NudgeItem."""
    item.field, item.kind, item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = window


# ---- staging --------------------------------------------------------------------------------------------------------------------
def staging(elements, dtype, device, alias_on_cpu=False):
    """(device buffer, host buffer) of `elements` each; the host's is pinned where there is a device.  On the CPU they are two
    tensors, or ONE with `alias_on_cpu` (then there is nothing to copy)."""
    device = torch.device(device)
    dev = torch.empty(elements, dtype=dtype, device=device)
    if device.type == "cpu":
        return dev, dev if alias_on_cpu else torch.empty(elements, dtype=dtype)
    return dev, torch.empty(elements, dtype=dtype, pin_memory=True)


def to_device(staging, staged):
    """The one host-to-device copy of a call (on the current stream: the launch that reads it follows it there); none where
    the two are one tensor (staging's alias_on_cpu)."""
    if staged is not staging:
        staged.copy_(staging, non_blocking=True)


def to_host(packed, host):
    """The one device-to-host copy of a call (on the current stream, behind the launch that wrote it) and the one wait for it."""
    host.copy_(packed, non_blocking=True)
    wait_for(packed.device)


def upload_table(arr, device):
    """A ctypes table on the device: through a pinned staging array on the launch stream (no synchronisation).  Returns the
    tensors to keep alive with the table (device copy first; on the CPU the one tensor twice)."""
    dev, stage = staging(C.sizeof(arr), torch.uint8, device, alias_on_cpu=True)
    C.memmove(stage.data_ptr(), arr, C.sizeof(arr))
    to_device(stage, dev)
    return dev, stage


def chunks(seq, n):
    """(first, seq[first:first + n]) for the launches of at most n entries each."""
    for first in range(0, len(seq), n):
        yield first, seq[first:first + n]
