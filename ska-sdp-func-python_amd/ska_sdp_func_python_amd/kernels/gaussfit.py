"""Batched 2-D Gaussian fits for fit_skycomponent (csrc/gaussfit.hip)."""

import ctypes

import torch

from .. import _lib
from ._operands import DT_CODE, alloc, on_gpu, ptr, ptr_table, stream

GAUSS_FIT_WINDOW = _lib.SDP_HIP_GAUSS_FIT_WINDOW
GAUSS_FIT_STATUS = {0: "converged", 1: "max_iter reached", 2: "not finite"}


def gauss_fit(planes, x0, y0, max_iter=100):
    """Least-squares fits of a rotated 2-D Gaussian to windows of
    GAUSS_FIT_WINDOW x GAUSS_FIT_WINDOW pixels, all in one kernel launch.

    ``planes`` is a list of 2-D device tensors, one per fit (float32 or
    float64, one dtype and one device for the call, last stride 1): views
    into a cube or images of their own, of any sizes; a plane may be given
    for many fits.  Fit f reads the window whose first pixel is row ``y0[f]``,
    column ``x0[f]`` of ``planes[f]``; a window that does not lie wholly on its
    plane raises ``ValueError``.  The planes are only read.

    Returns device tensors ``params`` [nfit, 6] float64 (amplitude, x_mean,
    y_mean, x_stddev, y_stddev, theta of astropy's Gaussian2D, the means in the
    plane's pixel coordinates), ``status`` [nfit] int32 (0 converged, 1
    ``max_iter`` model evaluations reached, 2 a pixel or an iterate was not
    finite: params NaN) and ``niter`` [nfit] int32 (model evaluations).  The
    start is the reference's (amplitude max z, means at the window centre,
    standard deviations 1, theta 0) and the solver Levenberg-Marquardt in fp64
    (csrc/gaussfit.hip).  A fit's result depends on its own window alone."""
    import numpy as np
    planes = list(planes)
    nfit = len(planes)
    x0 = np.asarray(x0).reshape(-1)
    y0 = np.asarray(y0).reshape(-1)
    if len(x0) != nfit or len(y0) != nfit:
        raise ValueError(f"gauss_fit: {nfit} planes, {len(x0)} x0 and {len(y0)} y0")
    if not (np.issubdtype(x0.dtype, np.integer) and np.issubdtype(y0.dtype, np.integer)) and nfit:
        raise ValueError("gauss_fit: x0 and y0 must be integers")
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError("gauss_fit: max_iter must be at least 1")
    if nfit == 0:
        dev = torch.device("cuda", torch.cuda.current_device())
        return (torch.empty((0, 6), dtype=torch.float64, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))
    first = on_gpu(planes[0], "planes")
    if first.dtype not in (torch.float32, torch.float64):
        raise ValueError("gauss_fit: the planes must be float32 or float64")
    strides = np.empty(nfit, dtype=np.int64)
    seen = {}
    for f, t in enumerate(planes):
        key = id(t)
        if key not in seen:
            on_gpu(t, "planes")
            if t.dim() != 2 or t.dtype != first.dtype or t.device != first.device:
                raise ValueError("gauss_fit: the planes must be 2-D and agree in dtype and device")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("gauss_fit: the x stride of every plane must be 1")
            if t.stride(0) < 0:
                raise ValueError("gauss_fit: a row stride is negative")
            seen[key] = (t.stride(0), int(t.shape[0]), int(t.shape[1]))
        strides[f], ny, nx = seen[key]
        if not (0 <= x0[f] and x0[f] + GAUSS_FIT_WINDOW <= nx
                and 0 <= y0[f] and y0[f] + GAUSS_FIT_WINDOW <= ny):
            raise ValueError(f"gauss_fit: the window of fit {f} at row {y0[f]}, column {x0[f]} "
                             f"does not lie on its plane of {ny} x {nx} pixels")
    x0 = np.ascontiguousarray(x0, dtype=np.int32)
    y0 = np.ascontiguousarray(y0, dtype=np.int32)
    dev = first.device
    params = alloc((nfit, 6), torch.float64, dev)
    status = torch.empty(nfit, dtype=torch.int32, device=dev)
    niter = torch.empty(nfit, dtype=torch.int32, device=dev)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_gauss_fit", nfit, ptr_table(planes), DT_CODE[first.dtype],
                  host(strides), host(x0), host(y0), max_iter, ptr(params), ptr(status),
                  ptr(niter), stream(dev))
    return params, status, niter
