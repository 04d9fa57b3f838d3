"""Weighted sums over stacks of image planes and clean thresholds
(csrc/taylor.hip, csrc/imgsum.hip): sdp_hip_mix_planes / sum_planes / peak_abs."""

import ctypes

import torch

from .. import _lib
from ._operands import (DT_CODE, alloc, byte_ranges, dev_array, on_gpu, overlaps, plane_list, ptr,
                        ptr_table)
from ._operands import stream as _stream  # (mix_planes has a parameter named stream)

# planes the kernel holds in registers per pixel: with min(nin, nout) at most
# this, every plane is read once and written once
MIX_PLANES_REGS = _lib.SDP_HIP_MIX_PLANES_REGS
MIX_PLANES_MAX = _lib.SDP_HIP_MIX_PLANES_MAX
MIX_NAN_INPUT = _lib.SDP_HIP_MIX_NAN_INPUT
MIX_NAN_OUTPUT = _lib.SDP_HIP_MIX_NAN_OUTPUT
SUM_PLANES_MAX = _lib.SDP_HIP_SUM_PLANES_MAX
PEAK_NAN_INPUT = _lib.SDP_HIP_PEAK_NAN_INPUT
PEAK_NAN_MEAN = _lib.SDP_HIP_PEAK_NAN_MEAN
_PEAK_MODES = {"moment0": _lib.SDP_HIP_PEAK_MOMENT0, "refchan": _lib.SDP_HIP_PEAK_REFCHAN}


def mix_planes(inputs, weights, outputs=None, check_nan=False, stream=None):
    """out[k] = sum_c weights[k, c] * inputs[c] over a stack of image planes:
    every output element starts from +0.0 and adds its terms in ascending c,
    the product and the sum each rounded once in float64 (numpy's
    ``out[k] += inputs[c] * w``, bit for bit).

    ``inputs`` and ``outputs`` are cubes (planes along the first axis) or
    lists of device tensors, which may be separately allocated or slices of a
    cube; every plane is contiguous and they all hold the same number of
    elements.  The inputs are all float32 or all float64, the outputs
    float64; without ``outputs`` a float64 cube [nout, *inputs[0].shape] is
    allocated.  ``weights`` is a host array [nout, nin].  No output may
    overlap an input or another output.  ``stream`` (a torch stream or a raw
    handle) defaults to torch's current stream.

    Returns the outputs; with ``check_nan`` the call waits for the stream and
    returns (outputs, flags), flags the sum of MIX_NAN_INPUT (a NaN was read)
    and MIX_NAN_OUTPUT (a NaN was written), 0 on clean data."""
    import numpy as np
    ins = plane_list(inputs, "inputs")
    if not ins:
        raise ValueError("mix_planes needs at least one input plane")
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != len(ins) or w.shape[0] < 1:
        raise ValueError(f"weights must be [nout, nin = {len(ins)}], not {w.shape}")
    nout, nin = w.shape
    if max(nin, nout) > MIX_PLANES_MAX:
        raise ValueError(f"mix_planes takes at most {MIX_PLANES_MAX} input and as many output "
                         f"planes, not {nin} and {nout}")
    first = on_gpu(ins[0], "inputs")
    dev, npix = first.device, first.numel()
    if first.dtype not in (torch.float32, torch.float64) or npix < 1:
        raise ValueError("the input planes must be non-empty float32 or float64 tensors")
    for p in ins:
        on_gpu(p, "inputs")
        if p.dtype != first.dtype or p.device != dev or p.numel() != npix:
            raise ValueError("the input planes must agree in dtype, device and size")
        if not p.is_contiguous():
            raise ValueError("every input plane must be contiguous")
    result = outputs
    if outputs is None:
        result = outputs = alloc((nout,) + tuple(first.shape), torch.float64, dev)
    outs = plane_list(outputs, "outputs")
    if len(outs) != nout:
        raise ValueError(f"{len(outs)} output planes for {nout} rows of weights")
    for p in outs:
        on_gpu(p, "outputs")
        if p.dtype != torch.float64 or p.device != dev or p.numel() != npix:
            raise ValueError("the output planes must be float64 on the inputs' device and of "
                             "their size")
        if not p.is_contiguous():
            raise ValueError("every output plane must be contiguous")
    i_lo, i_hi = byte_ranges(ins)
    o_lo, o_hi = byte_ranges(outs)
    if overlaps(o_lo[:, None], o_hi[:, None], i_lo[None, :], i_hi[None, :]).any():
        raise ValueError("an output plane overlaps an input plane")
    order = np.argsort(o_lo)
    if (o_hi[order][:-1] > o_lo[order][1:]).any():
        raise ValueError("two output planes overlap")
    seen = ctypes.c_int(0)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_mix_planes", nin, nout, npix, ptr_table(ins), DT_CODE[first.dtype],
                  ptr_table(outs), ctypes.c_void_p(w.ctypes.data),
                  ctypes.byref(seen) if check_nan else ctypes.POINTER(ctypes.c_int)(),
                  _stream(dev, stream))
    return (result, seen.value) if check_nan else result


def _real_view(t):
    return torch.view_as_real(t) if t.is_complex() else t


def sum_planes(inputs, weights=None, sumwt=None, normalise=True, out=None):
    """One tensor from a list of device tensors of one shape and dtype, in one
    launch that reads every input once and writes the output once.

    With ``weights`` [N, *lead] (host, float64), ``lead`` the leading axes of
    the inputs that index their planes ([nchan, npol] of image cubes):
    out[p] = sum_n weights[n, p] * inputs[n][p], every element from +0.0 in
    list order, product and sum each rounded once in float64; with
    ``normalise`` the element is then divided by ``sumwt`` [*lead] where that
    is positive and set to +0.0 where it is not, whatever the sum (NaN
    included).  For float64 that is numpy's ``im += w[..., None, None] * x``
    over the list and the reference's normalise_sumwt, bit for bit; a float32
    result is rounded once, from the float64 value.  Float32 or float64.

    Without ``weights``: out = inputs[0] + inputs[1] + ... in the element
    type and list order, numpy's ``a += b``; complex64 and complex128 are
    summed on their real views.  ``out`` may then be ``inputs[0]`` itself.

    An input that is not contiguous is copied; ``out`` (default: a new tensor)
    has the inputs' shape and dtype, is contiguous and overlaps no input
    otherwise.  Returns ``out``; the call only enqueues work."""
    import numpy as np
    ins = list(inputs)
    if not 1 <= len(ins) <= SUM_PLANES_MAX:
        raise ValueError(f"sum_planes takes 1 .. {SUM_PLANES_MAX} inputs, not {len(ins)}")
    first = on_gpu(ins[0], "inputs")
    dev, shape, dtype = first.device, tuple(first.shape), first.dtype
    real = (torch.float32, torch.float64)
    if dtype not in (real if weights is not None else real + (torch.complex64, torch.complex128)) \
            or first.numel() < 1:
        raise ValueError("the inputs must be non-empty float32 or float64 tensors (or, without "
                         "weights, complex64 or complex128)")
    for t in ins:
        on_gpu(t, "inputs")
        if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape:
            raise ValueError("the inputs must agree in dtype, device and shape")
    if out is None:
        out = alloc(shape, dtype, dev)
    on_gpu(out, "out")
    if out.dtype != dtype or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor of the inputs' dtype, device and shape")
    cubes = [_real_view(t.contiguous()) for t in ins]
    res = _real_view(out)
    nelem = res.numel()
    if weights is None:
        if sumwt is not None:
            raise ValueError("sumwt is used with weights only")
        nplane, w_dev, s_dev, norm = 1, None, None, 0
    else:
        w = np.array(weights, dtype=np.float64)  # a copy: torch takes no read-only array
        lead = w.shape[1:]
        if w.ndim < 1 or w.shape[0] != len(ins) or lead != shape[:len(lead)]:
            raise ValueError(f"weights must be [{len(ins)}, leading axes of {shape}], not {w.shape}")
        nplane = int(np.prod(lead, dtype=np.int64))
        w_dev = dev_array(w.reshape(len(ins), nplane), np.float64, dev)
        norm, s_dev = int(bool(normalise)), None
        if norm:
            if sumwt is None:
                raise ValueError("normalising needs sumwt")
            s = np.array(sumwt, dtype=np.float64)
            if s.shape != lead:
                raise ValueError(f"sumwt must be {lead}, not {s.shape}")
            s_dev = dev_array(s.reshape(nplane), np.float64, dev)
    clash = overlaps(*byte_ranges([res]), *byte_ranges(cubes))
    if weights is None and cubes[0].data_ptr() == res.data_ptr():
        clash[0] = False  # the sum onto its first entry
    if clash.any():
        raise ValueError("out overlaps an input")
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_sum_planes", len(cubes), nplane, nelem // nplane, ptr_table(cubes),
                  DT_CODE[res.dtype], ptr(res), ptr(w_dev), ptr(s_dev), norm, _stream(dev))
    return out


def peak_abs(cube, mode="moment0"):
    """The largest magnitude of a device cube [nchan, npol, ny, nx] (float32
    or float64): with mode "moment0" of its channel mean, max |(sum_c x[c]) /
    nchan| with the sum in float64 in channel order, with "refchan" of channel
    nchan // 2.  The cube may be any view whose x stride is 1 -- a facet of a
    larger image is read where it lies.  Returns (peak, flags): a Python float
    and 0 or the sum of PEAK_NAN_INPUT (a NaN was read) and PEAK_NAN_MEAN (a
    channel mean was NaN).  "refchan" gives NaN when it read one, as
    numpy.max does; "moment0" gives the peak of the means that are not NaN.
    The call waits for the stream."""
    on_gpu(cube, "cube")
    if mode not in _PEAK_MODES:
        raise ValueError(f"mode must be one of {sorted(_PEAK_MODES)}, not {mode!r}")
    if cube.dim() != 4 or cube.numel() < 1 or cube.dtype not in (torch.float32, torch.float64):
        raise ValueError("the cube must be a non-empty float32 or float64 tensor "
                         "[nchan, npol, ny, nx]")
    nchan, npol, ny, nx = cube.shape
    cs, ps, rs, xs = cube.stride()
    if nx > 1 and xs != 1:
        raise ValueError("the x axis of the cube must be contiguous")
    if max(nchan, npol, ny, nx) >= 2 ** 31:
        raise ValueError("cube axes of 2^31 elements or more are not supported")
    peak, seen = ctypes.c_double(0.0), ctypes.c_int(0)
    with torch.cuda.device(cube.device):
        _lib.call("sdp_hip_peak_abs", _PEAK_MODES[mode], nchan, npol, ny, nx, ptr(cube),
                  DT_CODE[cube.dtype], cs, ps, rs, ctypes.byref(peak), ctypes.byref(seen),
                  _stream(cube.device))
    value = peak.value
    if mode == "refchan" and seen.value & PEAK_NAN_INPUT:
        value = float("nan")
    return value, seen.value
