"""Image segmentation for find_skycomponents (csrc/segment.hip): sdp_hip_segment_*."""

import ctypes

import torch

from .. import _lib
from ._operands import DT_CODE, alloc, on_gpu, ptr, stream

SEGMENT_KERNEL_MAX = _lib.SDP_HIP_SEGMENT_KERNEL_MAX


def _segment_planes(planes, name):
    """The planes [nplanes, ny, nx] of a segmentation call: a float32 or float64
    device tensor whose planes are contiguous and evenly spaced, such as a cube
    or ``pixels[:, 0]`` of an image."""
    on_gpu(planes, name)
    if planes.dim() != 3 or planes.dtype not in (torch.float32, torch.float64) \
            or planes.numel() == 0:
        raise ValueError(f"{name} must be a non-empty float32 or float64 device tensor "
                         "[nplanes, ny, nx]")
    nplanes, ny, nx = (int(n) for n in planes.shape)
    if ny * nx >= 2 ** 31:
        raise ValueError("image planes of 2^31 pixels or more are not supported")
    if not planes[0].is_contiguous() or (nplanes > 1 and planes.stride(0) < ny * nx):
        planes = planes.contiguous()
    return planes, nplanes, ny, nx, (planes.stride(0) if nplanes > 1 else ny * nx)


def segment_image(planes, threshold, npixels, kernel=None):
    """The segment map of the channel mean of ``planes`` [nchan, ny, nx]
    (float32 or float64, on the device): the mean in channel order and in the
    planes' type, smoothed in float64 by ``kernel`` (a host array [K, K], K odd
    and at most SEGMENT_KERNEL_MAX; pixels off the image count as 0 and the
    sum is divided by the kernel's; None: no smoothing), then the 8-connected
    components of ``smoothed > threshold`` that have at least ``npixels``
    pixels, numbered from 1 by their first pixel in raster order as
    scipy.ndimage.label numbers them; 0 is the background.

    Returns (labels, nlabels): an int32 device tensor [ny, nx] and the number
    of segments; the call waits for the device to learn it.  A pixel whose
    mean is not finite raises ``ValueError``."""
    import numpy as np
    planes, nchan, ny, nx, stride = _segment_planes(planes, "planes")
    taps = np.ones((1, 1)) if kernel is None else np.ascontiguousarray(kernel, dtype=np.float64)
    if taps.ndim != 2 or taps.shape[0] != taps.shape[1] or taps.shape[0] % 2 != 1:
        raise ValueError("the smoothing kernel must be square with an odd number of pixels a side")
    if taps.shape[0] > SEGMENT_KERNEL_MAX:
        raise ValueError(f"the smoothing kernel has {taps.shape[0]} pixels a side: at most "
                         f"{SEGMENT_KERNEL_MAX} are supported")
    tap_sum = float(taps.sum())
    if not (np.isfinite(taps).all() and tap_sum > 0.0):
        raise ValueError("the smoothing kernel must be finite with a positive sum")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("the threshold is NaN")
    dev = planes.device
    labels = alloc((ny, nx), torch.int32, dev)
    count = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    keep = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)  # non-finite flag, nlabels
    with torch.cuda.device(dev):
        st = stream(dev)
        _lib.call("sdp_hip_segment_label", nchan, ny, nx, ptr(planes), DT_CODE[planes.dtype],
                  stride, taps.shape[0], ctypes.c_void_p(taps.ctypes.data), tap_sum, threshold,
                  ptr(labels), ptr(count), ptr(state), st)
        _lib.call("sdp_hip_segment_roots", ny, nx, ptr(labels), ptr(count),
                  int(min(max(int(npixels), 0), 2 ** 31 - 1)), ptr(keep), st)
        rank = torch.cumsum(keep.view(-1), 0, dtype=torch.int32)
        _lib.call("sdp_hip_segment_relabel", ny, nx, ptr(labels), ptr(keep), ptr(rank),
                  ptr(labels), st)
        state[1] = rank[-1]
        nonfinite, nlabels = (int(v) for v in state.cpu())
    if nonfinite:
        raise ValueError("segment_image: the image has a pixel that is not finite")
    return labels, nlabels


def segment_peaks(planes, labels, nlabels):
    """Per plane and segment, the maximum of ``planes`` [nplanes, ny, nx] over
    the pixels of the segment map ``labels`` (int32 [ny, nx], segments 1 ..
    nlabels) and the flat index y * nx + x of the first pixel, in raster order,
    that has it: (values float64 [nplanes, nlabels], indices int64 [nplanes,
    nlabels]) on the device.  Exact and repeatable; -0.0 counts as 0.0."""
    planes, nplanes, ny, nx, stride = _segment_planes(planes, "planes")
    on_gpu(labels, "labels")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (ny, nx) \
            or not labels.is_contiguous() or labels.device != planes.device:
        raise ValueError("labels must be a contiguous int32 tensor [ny, nx] on the planes' device")
    nlabels = int(nlabels)
    if not 0 <= nlabels < 2 ** 31:
        raise ValueError("bad number of segments")
    dev = planes.device
    values = torch.empty((nplanes, nlabels), dtype=torch.float64, device=dev)
    indices = torch.empty((nplanes, nlabels), dtype=torch.int64, device=dev)
    if nlabels:
        with torch.cuda.device(dev):
            _lib.call("sdp_hip_segment_peaks", nplanes, ny, nx, ptr(planes),
                      DT_CODE[planes.dtype], stride, ptr(labels), nlabels, ptr(values),
                      ptr(indices), stream(dev))
    return values, indices
