"""Oversampled w-projection kernels (csrc/wkernel.hip): sdp_hip_wkernel_create."""

import torch

from .. import _lib
from ._operands import alloc, on_gpu, ptr, stream


def wkernel_create(npixel, oversampling, support, w, field_of_view, taper=None, pb=None):
    """The convolution functions of the w planes ``w`` [nw] (float64, on the
    device; plane z is made for exactly the value w[z]) from a far field of
    ``npixel`` pixels a side across ``field_of_view`` (direction cosines), as
    include/ska_sdp_hip.h defines them: a new device tensor [npb, nw, nd, nd,
    support, support] complex128 with nd = 2 (oversampling // 2) + 1.

    ``taper`` [npixel] float64 multiplies the far field along both axes,
    ``pb`` [npb, npixel, npixel] complex128 pixel by pixel; None stands for
    ones, and npb is 1 without ``pb``.  Both on the device, contiguous."""
    on_gpu(w, "w")
    if w.dtype != torch.float64 or w.dim() != 1 or w.shape[0] < 1 or not w.is_contiguous():
        raise ValueError("w must be a contiguous float64 device tensor [nw] with nw >= 1")
    dev = w.device
    npixel, oversampling, support = int(npixel), int(oversampling), int(support)
    if support < 2 or support % 2:
        raise ValueError(f"support {support} must be even and at least 2")
    if npixel % 2 or npixel < support + 2:
        raise ValueError(f"npixel {npixel} must be even and at least support + 2 = {support + 2}")
    if oversampling < 1:
        raise ValueError(f"oversampling {oversampling} must be at least 1")
    if taper is not None:
        on_gpu(taper, "taper")
        if taper.dtype != torch.float64 or tuple(taper.shape) != (npixel,) \
                or not taper.is_contiguous() or taper.device != dev:
            raise ValueError(f"taper must be a contiguous float64 tensor [{npixel}] on w's device")
    npb = 1
    if pb is not None:
        on_gpu(pb, "pb")
        if pb.dtype != torch.complex128 or pb.dim() != 3 or pb.shape[0] < 1 \
                or tuple(pb.shape[1:]) != (npixel, npixel) or not pb.is_contiguous() \
                or pb.device != dev:
            raise ValueError(f"pb must be a contiguous complex128 tensor [npb, {npixel}, {npixel}] "
                             "on w's device")
        npb = int(pb.shape[0])
    nd = 2 * (oversampling // 2) + 1
    nw = int(w.shape[0])
    cf = alloc((npb, nw, nd, nd, support, support), torch.complex128, dev)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_wkernel_create", npixel, oversampling, support, nw, npb,
                  float(field_of_view), ptr(w), ptr(taper), ptr(pb), ptr(cf), stream(dev))
    return cf
