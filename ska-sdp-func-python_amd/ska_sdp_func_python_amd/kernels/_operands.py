"""What every kernel family's wrappers share: device checks, raw pointers,
allocation, dtype codes and the host buffers handed to the C ABI."""

import ctypes

import torch

from .. import _lib

DT_CODE = {
    torch.complex64: _lib.SDP_HIP_C64,
    torch.complex128: _lib.SDP_HIP_C128,
    torch.float32: _lib.SDP_HIP_F32,
    torch.float64: _lib.SDP_HIP_F64,
}

# bytes per element of the flag arrays the kernels read in place
FLAG_BYTES = {torch.int64: 8, torch.int32: 4, torch.int8: 1, torch.uint8: 1, torch.bool: 1}


def on_gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a device (HIP) tensor")
    return t


def stream(device, given=None):
    """torch's current stream on ``device``, or ``given`` (a torch stream or a
    raw handle), as the C ABI takes it."""
    if given is not None:
        return ctypes.c_void_p(getattr(given, "cuda_stream", given))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def alloc(shape, dtype, dev, may_release=True):
    """torch.empty on the device; when the caching allocator cannot serve it
    because the library's workspace holds the memory (cached w planes and
    records of an earlier large call), the workspace is released and the
    allocation retried once (the w planes are re-made on the next call).
    ``may_release=False`` (a batched invert past its first batch, whose
    resident planes hold the earlier batches' work) re-raises instead."""
    try:
        return torch.empty(shape, dtype=dtype, device=dev)
    except torch.OutOfMemoryError:
        if not may_release:
            raise
        _lib.call("sdp_hip_release_workspace")
        torch.cuda.empty_cache()
        return torch.empty(shape, dtype=dtype, device=dev)


def dev_array(a, dtype, dev):
    import numpy as np
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def check_uvw(uvw):
    on_gpu(uvw, "uvw")
    if uvw.dtype != torch.float64 or uvw.dim() != 2 or uvw.shape[1] != 3 or uvw.stride(1) != 1:
        raise ValueError("uvw must be float64 [nrow, 3] with unit column stride")


def vis4(t, name):
    on_gpu(t, name)
    if t.dtype not in (torch.complex64, torch.complex128) or t.dim() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous complex [t, b, f, p] tensor")
    return t


def flags_of(flags, shape):
    """(flags, bytes per flag) of a contiguous flag tensor of ``shape``, or
    (None, 0)."""
    if flags is None:
        return None, 0
    on_gpu(flags, "flags")
    if tuple(flags.shape) != tuple(shape) or not flags.is_contiguous() \
            or flags.dtype not in FLAG_BYTES:
        raise ValueError("flags must be a contiguous integer tensor shaped like vis")
    return flags, FLAG_BYTES[flags.dtype]


def f64_like(t, name, like):
    on_gpu(t, name)
    if t.shape != like.shape or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous float64 shaped like vis")
    return t


# The two helpers below return a bare c_void_p over a ctypes array made here.
# ctypes.cast keeps a reference to the object it casts (in the result's
# ``_objects``), so the array lives exactly as long as the returned pointer:
# a wrapper that holds the pointer until _lib.call returns -- in a local, or
# in the argument list itself -- keeps the buffer alive.  This is relied on
# deliberately (tests/test_kernels_operands_cpu.py reads both back after a
# collection).
def host_doubles(values, count=None):
    """``values`` as a host double[] for the C ABI (``count`` entries, by
    default one per value), or None for None."""
    if values is None:
        return None
    vals = [float(x) for x in values]
    buf = (ctypes.c_double * (len(vals) if count is None else count))(*vals)
    return ctypes.cast(buf, ctypes.c_void_p)


def ptr_table(tensors):
    """The device addresses of ``tensors`` as a host void*[] for the C ABI
    (with one spare NULL entry, so that an empty list still has storage)."""
    tab = (ctypes.c_void_p * (len(tensors) + 1))(*[t.data_ptr() for t in tensors])
    return ctypes.cast(tab, ctypes.c_void_p)


def plane_list(x, name):
    """The planes of a cube (its first axis) or of a list of tensors."""
    if isinstance(x, torch.Tensor):
        if x.dim() < 2:
            raise ValueError(f"{name}: a cube needs a plane axis in front of the pixel axes")
        return [x[i] for i in range(x.shape[0])]
    return list(x)


def byte_ranges(planes):
    import numpy as np
    start = np.array([p.data_ptr() for p in planes], dtype=np.uint64)
    return start, start + np.array([p.numel() * p.element_size() for p in planes], dtype=np.uint64)


def overlaps(lo_a, hi_a, lo_b, hi_b):
    """Where the byte ranges [lo_a, hi_a) and [lo_b, hi_b) meet (arrays
    broadcast against each other)."""
    return (lo_a < hi_b) & (lo_b < hi_a)
