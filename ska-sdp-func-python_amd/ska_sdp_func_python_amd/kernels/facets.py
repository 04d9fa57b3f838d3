"""Gather of image facets (csrc/facets.hip): sdp_hip_gather_facets."""

import ctypes

import torch

from .. import _lib
from ._operands import DT_CODE, alloc, on_gpu, ptr, ptr_table
from ._operands import stream as _stream  # (the wrappers have a parameter named stream)

GATHER_FACETS_MAX = _lib.SDP_HIP_GATHER_FACETS_MAX


def _gather_facets_call(tabs, facets, lead, facet_shape, image_shape, origin, step, taper_y,
                        taper_x, normalise, want_image, want_weights, dtype, dev, stream):
    """``tabs``: the facets' host tables (addresses, plane strides, row
    strides) as the C ABI takes them, or None to read no facet."""
    import numpy as np
    (dy, dx), (ny, nx) = facet_shape, image_shape
    (y0, x0), (sy, sx) = origin, step
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("the facets must be float32 or float64")
    if min(dy, dx, ny, nx) < 1 or dy > ny or dx > nx:
        raise ValueError(f"facets of {dy} x {dx} pixels do not fit an image of {ny} x {nx}")
    if sy < 1 or sx < 1:
        raise ValueError(f"the steps between facets must be at least 1, not {sy} and {sx}")
    if y0 < 0 or x0 < 0 or y0 + (facets - 1) * sy + dy > ny or x0 + (facets - 1) * sx + dx > nx:
        raise ValueError("the facets leave the image")
    if (taper_y is None) != (taper_x is None):
        raise ValueError("taper_y and taper_x come together or not at all")
    tapers = []
    for taper, n in ((taper_y, dy), (taper_x, dx)):
        if taper is not None:
            taper = np.ascontiguousarray(taper, dtype=np.float64)
            if taper.shape != (n,):
                raise ValueError(f"a taper of shape {taper.shape} for a facet side of {n}")
        tapers.append(taper)
    nplanes = 1
    for n in lead:
        nplanes *= int(n)
    if nplanes < 1:
        raise ValueError("the image has no planes")
    shape = tuple(lead) + (ny, nx)
    out = alloc(shape, dtype, dev) if want_image else None
    sumwt = alloc(shape, dtype, dev) if want_weights else None
    null = ctypes.c_void_p(0)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_gather_facets", DT_CODE[dtype], int(facets), nplanes, int(ny), int(nx),
                  int(dy), int(dx), int(y0), int(x0), int(sy), int(sx),
                  *([null] * 3 if tabs is None else tabs),
                  *[null if t is None else ctypes.c_void_p(t.ctypes.data) for t in tapers],
                  int(bool(normalise)), ptr(out), ptr(sumwt), _stream(dev, stream))
    return out, sumwt


def gather_facets(facet_list, facets, image_shape, origin, step, taper_y=None, taper_x=None,
                  normalise=False, weights=False, stream=None):
    """An image from ``facets`` x ``facets`` overlapping sub-images in one
    pass: every facet pixel is read once, every output pixel written once.

    ``facet_list`` holds facets**2 device tensors [..., dy, dx] in fy-major
    order, all of one shape, dtype (float32 or float64) and device; facet
    (fy, fx) lies with its first pixel at ``origin + (fy, fx) * step`` of the
    image of ``image_shape`` = (ny, nx).  A facet may be a view of a larger
    image: its x stride must be 1 and its planes (the leading axes) evenly
    spaced, nothing more.  ``taper_y`` [dy] and ``taper_x`` [dx] are host
    arrays (float64), or both None for weights of 1.

    Per output element, over the facets that cover it in ascending fy, then
    ascending fx, in the facets' dtype: ``wt = dtype(taper_y[j] * taper_x[i])``,
    ``acc += wt * v``, ``sum += wt``; the result is ``acc / sum`` (0 where
    ``sum <= 0``) with ``normalise``, else ``acc`` -- numpy's results for the
    reference's image_gather_facets with and without an overlap, bit for bit.
    An uncovered pixel gets +0.

    Returns the new image [..., ny, nx]; with ``weights`` also the summed
    weights (ones without ``normalise``, as the reference's flat).  ``stream``
    (a torch stream or a raw handle) defaults to torch's current stream."""
    import numpy as np
    facet_list = list(facet_list)
    facets = int(facets)
    if not 1 <= facets <= GATHER_FACETS_MAX:
        raise ValueError(f"gather_facets takes 1 .. {GATHER_FACETS_MAX} facets per axis, "
                         f"not {facets}")
    if len(facet_list) != facets * facets:
        raise ValueError(f"{len(facet_list)} facets given for a raster of {facets} x {facets}")
    first = on_gpu(facet_list[0], "facet_list")
    if first.dim() < 3:
        raise ValueError("a facet needs a plane axis in front of its two pixel axes")
    lead, nlead = tuple(first.shape[:-2]), first.dim() - 2
    pstrides = np.empty(len(facet_list), dtype=np.int64)
    rstrides = np.empty(len(facet_list), dtype=np.int64)
    for f, t in enumerate(facet_list):
        on_gpu(t, "facet_list")
        if t.dtype != first.dtype or t.device != first.device or t.shape != first.shape:
            raise ValueError("the facets must agree in dtype, device and shape")
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise ValueError("the x stride of every facet must be 1")
        # the planes in C order of the leading axes, one stride apart
        pstride = 0
        for a in range(nlead - 1, -1, -1):
            if t.shape[a] > 1:
                pstride = t.stride(a)
                break
        span = pstride
        for a in range(nlead - 1, -1, -1):
            if t.shape[a] > 1 and t.stride(a) != span:
                raise ValueError("the planes of every facet must be evenly spaced in memory")
            span *= t.shape[a]
        if pstride < 0 or t.stride(-2) < 0:
            raise ValueError("a facet stride is negative")
        pstrides[f], rstrides[f] = pstride, t.stride(-2)
    tabs = (ptr_table(facet_list), ctypes.c_void_p(pstrides.ctypes.data),
            ctypes.c_void_p(rstrides.ctypes.data))
    out, sumwt = _gather_facets_call(tabs, facets, lead, first.shape[-2:], image_shape, origin,
                                     step, taper_y, taper_x, normalise, True, weights,
                                     first.dtype, first.device, stream)
    return (out, sumwt) if weights else out


def gather_facet_weights(facets, lead_shape, facet_shape, image_shape, origin, step, dtype, device,
                         taper_y=None, taper_x=None, normalise=True, stream=None):
    """The summed weights of ``gather_facets`` alone, [*lead_shape, ny, nx] of
    ``dtype`` on ``device``: no facet is read."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("device must be a HIP device")
    if not 1 <= int(facets) <= GATHER_FACETS_MAX:
        raise ValueError(f"gather_facets takes 1 .. {GATHER_FACETS_MAX} facets per axis, "
                         f"not {facets}")
    return _gather_facets_call(None, int(facets), tuple(lead_shape), facet_shape, image_shape, origin,
                               step, taper_y, taper_x, normalise, False, True, dtype, dev,
                               stream)[1]
