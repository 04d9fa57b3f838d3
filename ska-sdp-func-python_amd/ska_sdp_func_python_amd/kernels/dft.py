"""Sky-component DFT and its adjoint (csrc/dft.hip, csrc/idft.hip)."""

import torch

from .. import _lib
from ._operands import DT_CODE, FLAG_BYTES, alloc, on_gpu, ptr, stream


def dft_point(direction_cosines, fluxes, uvw, freq=None, out=None, vis_dtype=torch.complex64):
    """Sky-component DFT on device.

    direction_cosines [ncomp,3] f64, fluxes [ncomp, 1|nchan, npol] c128.
    With ``freq`` given, ``uvw`` is [nrow,3] metres (lambda scaling fused);
    otherwise ``uvw`` is uvw_lambda [nrow, nchan, 3] (dft_point_v00 layout).
    Returns vis [nrow, nchan, npol].
    """
    dc = on_gpu(direction_cosines, "direction_cosines").to(torch.float64).contiguous()
    fl = on_gpu(fluxes, "fluxes").to(torch.complex128).contiguous()
    if fl.dim() != 3 or dc.dim() != 2 or dc.shape[1] != 3 or fl.shape[0] != dc.shape[0]:
        raise ValueError("direction_cosines [ncomp,3] and fluxes [ncomp,nchan,npol] required")
    ncomp, fnchan, npol = fl.shape
    uvw = on_gpu(uvw, "uvw").to(torch.float64).contiguous()
    if freq is not None:
        freq = on_gpu(freq, "freq").to(torch.float64).contiguous()
        nrow, nchan = uvw.shape[0], freq.shape[0]
    else:
        nrow, nchan = uvw.shape[0], uvw.shape[1]
    if out is None:
        out = alloc((nrow, nchan, npol), vis_dtype, uvw.device)
    if not out.is_contiguous() or tuple(out.shape) != (nrow, nchan, npol):
        raise ValueError("vis out must be contiguous [nrow, nchan, npol]")
    if freq is not None:
        _lib.call("sdp_hip_dft_point_metres", ncomp, ptr(dc), ptr(fl), fnchan, npol, nrow, nchan,
                  ptr(uvw), ptr(freq), ptr(out), DT_CODE[out.dtype], stream(uvw.device))
    else:
        _lib.call("sdp_hip_dft_point_v00", ncomp, ptr(dc), ptr(fl), fnchan, npol, nrow, nchan,
                  ptr(uvw), ptr(out), DT_CODE[out.dtype], stream(uvw.device))
    return out


def idft_point(direction_cosines, vis, weight, uvw, freq=None, flags=None, out=None):
    """Inverse sky-component DFT on device: the adjoint of ``dft_point``.

    direction_cosines [ncomp,3] f64; vis [nrow, nchan, npol] c64 or c128;
    weight f64 and flags (integers, 0/1, or None) shaped like vis.  With
    ``freq`` given, ``uvw`` is [nrow,3] metres (lambda scaling fused);
    otherwise ``uvw`` is uvw_lambda [nrow, nchan, 3].
    Returns (flux_sum [ncomp, nchan, npol] c128, sumwt [nchan, npol] f64):
    sum_row w (1-flag) vis exp(+2 pi i ...) and sum_row w (1-flag), both
    unnormalised (the reference's flux is flux_sum / sumwt where sumwt > 0).
    ``out`` = (flux_sum, sumwt) writes into caller-allocated tensors.
    """
    dc = on_gpu(direction_cosines, "direction_cosines").to(torch.float64).contiguous()
    if dc.dim() != 2 or dc.shape[1] != 3:
        raise ValueError("direction_cosines [ncomp,3] required")
    vis = on_gpu(vis, "vis")
    if vis.dtype not in (torch.complex64, torch.complex128) or vis.dim() != 3:
        raise ValueError("vis must be complex64 or complex128 [nrow, nchan, npol]")
    vis = vis.contiguous()
    nrow, nchan, npol = vis.shape
    weight = on_gpu(weight, "weight").to(torch.float64).contiguous()
    if tuple(weight.shape) != (nrow, nchan, npol):
        raise ValueError("weight must be shaped like vis")
    fb = 0
    if flags is not None:
        flags = on_gpu(flags, "flags").contiguous()
        if tuple(flags.shape) != (nrow, nchan, npol) or flags.dtype not in FLAG_BYTES:
            raise ValueError("flags must be an integer tensor shaped like vis")
        fb = FLAG_BYTES[flags.dtype]
    uvw = on_gpu(uvw, "uvw").to(torch.float64).contiguous()
    if freq is not None:
        freq = on_gpu(freq, "freq").to(torch.float64).contiguous()
        if tuple(uvw.shape) != (nrow, 3) or tuple(freq.shape) != (nchan,):
            raise ValueError("uvw [nrow,3] metres and freq [nchan] must match vis")
    elif tuple(uvw.shape) != (nrow, nchan, 3):
        raise ValueError("uvw_lambda [nrow, nchan, 3] must match vis")
    ncomp = dc.shape[0]
    if out is None:
        out = (alloc((ncomp, nchan, npol), torch.complex128, vis.device),
               alloc((nchan, npol), torch.float64, vis.device))
    flux_sum, sumwt = out
    if (not flux_sum.is_contiguous() or tuple(flux_sum.shape) != (ncomp, nchan, npol)
            or flux_sum.dtype != torch.complex128 or not sumwt.is_contiguous()
            or tuple(sumwt.shape) != (nchan, npol) or sumwt.dtype != torch.float64):
        raise ValueError("out must be contiguous (flux_sum [ncomp, nchan, npol] complex128, "
                         "sumwt [nchan, npol] float64)")
    if freq is not None:
        _lib.call("sdp_hip_idft_point_metres", ncomp, ptr(dc), npol, nrow, nchan, ptr(uvw),
                  ptr(freq), ptr(vis), DT_CODE[vis.dtype], ptr(weight), ptr(flags), fb,
                  ptr(flux_sum), ptr(sumwt), stream(vis.device))
    else:
        _lib.call("sdp_hip_idft_point_v00", ncomp, ptr(dc), npol, nrow, nchan, ptr(uvw),
                  ptr(vis), DT_CODE[vis.dtype], ptr(weight), ptr(flags), fb,
                  ptr(flux_sum), ptr(sumwt), stream(vis.device))
    return flux_sum, sumwt
