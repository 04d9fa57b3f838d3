"""Visibility operations (csrc/visops.hip): sdp_hip_vis_average_channels /
to_stokes / remove_continuum."""

import ctypes

import torch

from .. import _lib
from ._operands import DT_CODE, f64_like, flags_of, on_gpu, ptr, stream, vis4

MAX_CONTINUUM_DEGREE = 5


def _flags_required(flags, vis):
    if flags is None:
        raise ValueError("flags are required")
    return flags_of(flags, vis.shape)


def _like_outputs(vis, fl, shape):
    """New (vis, weight, imaging_weight, flags) of ``shape`` on vis's device."""
    dev = vis.device
    return (torch.empty(shape, dtype=vis.dtype, device=dev),
            torch.empty(shape, dtype=torch.float64, device=dev),
            torch.empty(shape, dtype=torch.float64, device=dev),
            torch.empty(shape, dtype=fl.dtype, device=dev))


def vis_average_channels(vis, weight, imaging_weight, flags, group, variant):
    """Weighted channel averages over groups of ``group`` channels (which must
    divide nchan) of device arrays [t, b, f, p]: (vis, weight, imaging_weight,
    flags) shaped [t, b, f / group, p].  variant 0 is
    integrate_visibility_by_channel's arithmetic, 1
    average_visibility_by_channel's (include/ska_sdp_hip.h)."""
    vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if group is None or int(group) != group or group < 1 or nchan % int(group):
        raise ValueError(f"the number of channels to average ({group}) must divide nchan = {nchan}")
    group = int(group)
    f64_like(weight, "weight", vis)
    f64_like(imaging_weight, "imaging_weight", vis)
    fl, fb = _flags_required(flags, vis)
    ov, ow, oiw, ofl = _like_outputs(vis, fl, (nt, nbl, nchan // group, npol))
    _lib.call("sdp_hip_vis_average_channels", nt * nbl, nchan, npol, group, int(variant),
              ptr(vis), DT_CODE[vis.dtype], ptr(weight), ptr(imaging_weight), ptr(fl), fb,
              ptr(ov), ptr(ow), ptr(oiw), ptr(ofl), fb, stream(vis.device))
    return ov, ow, oiw, ofl


def vis_to_stokes(vis, flags, matrix):
    """convert_visibility_to_stokes in place on device vis / flags [t, b, f, 4]:
    vis <- matrix @ vis per sample (matrix: 4 x 4 complex, host), every pol's
    flag <- flag[0] | flag[3]."""
    import numpy as np
    vis4(vis, "vis")
    if vis.shape[3] != 4:
        raise ValueError("stokesIQUV needs 4 polarisations")
    fl, fb = _flags_required(flags, vis)
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.complex128))
    if m.shape != (4, 4):
        raise ValueError("the conversion matrix must be 4 x 4")
    _lib.call("sdp_hip_vis_to_stokes", vis.numel() // 4, 4, _lib.SDP_HIP_STOKES_IQUV, ptr(vis),
              DT_CODE[vis.dtype], None, None, ptr(fl), fb, ctypes.c_void_p(m.ctypes.data),
              None, None, None, None, fb, stream(vis.device))
    return vis, fl


def vis_to_stokes_i(vis, weight, imaging_weight, flags):
    """convert_visibility_to_stokesI of device arrays [t, b, f, p] (p 2 or 4):
    new (vis, weight, imaging_weight, flags) shaped [t, b, f, 1]."""
    vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if npol not in (2, 4):
        raise ValueError("stokesI needs 2 or 4 polarisations")
    f64_like(weight, "weight", vis)
    f64_like(imaging_weight, "imaging_weight", vis)
    fl, fb = _flags_required(flags, vis)
    ov, ow, oiw, ofl = _like_outputs(vis, fl, (nt, nbl, nchan, 1))
    _lib.call("sdp_hip_vis_to_stokes", nt * nbl * nchan, npol, _lib.SDP_HIP_STOKES_I, ptr(vis),
              DT_CODE[vis.dtype], ptr(weight), ptr(imaging_weight), ptr(fl), fb, None,
              ptr(ov), ptr(ow), ptr(oiw), ptr(ofl), fb, stream(vis.device))
    return ov, ow, oiw, ofl


def vis_remove_continuum(vis, weight, flags, x, degree, mask=None, rank_capacity=None):
    """Fit and subtract a polynomial of ``degree`` in ``x`` [nchan] per
    (time, baseline, pol) spectrum, in place on device vis [t, b, f, p]
    (include/ska_sdp_hip.h).  Returns (deficient, count): the sorted indices
    row * npol + pol of the spectra with 1 <= n_live <= degree, which were
    left untouched, and their number; ``deficient`` is None when more than
    ``rank_capacity`` (default 2^20) were found."""
    vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if not 0 <= int(degree) <= MAX_CONTINUUM_DEGREE:
        raise ValueError(f"degree {degree}: the device fit takes degrees 0 to "
                         f"{MAX_CONTINUUM_DEGREE}")
    if nchan < 2:
        raise ValueError("remove_continuum needs at least 2 channels")
    f64_like(weight, "weight", vis)
    fl, fb = flags_of(flags, vis.shape)
    dev = vis.device
    on_gpu(x, "x")
    if x.dtype != torch.float64 or tuple(x.shape) != (nchan,) or not x.is_contiguous():
        raise ValueError("x must be contiguous float64 [nchan]")
    if mask is not None:
        on_gpu(mask, "mask")
        if tuple(mask.shape) != (nchan,):
            raise ValueError("mask must be [nchan]")
        mask = mask.to(torch.uint8).contiguous()
    nspec = nt * nbl * npol
    cap = 1 << 20 if rank_capacity is None else int(rank_capacity)
    cap = max(0, min(cap, nspec, 2 ** 31 - 1))
    rank_list = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.call("sdp_hip_vis_remove_continuum", nt * nbl, nchan, npol, ptr(vis),
              DT_CODE[vis.dtype], ptr(weight), ptr(fl), fb, ptr(x), ptr(mask), int(degree),
              ptr(rank_list), cap, ptr(count), stream(dev))
    n = int(count.item())
    if n > cap:
        return None, n
    return torch.sort(rank_list[:n]).values, n
