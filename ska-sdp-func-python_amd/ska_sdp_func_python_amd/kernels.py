"""Tensor-level wrappers over the C ABI (device buffers are torch tensors).

These are the thin host shims between the reference-shaped Python API
(imaging/, calibration/, grid_data/) and libska_sdp_hip.so.  They validate
shapes, dtypes and devices, pass raw device pointers + element strides, and
enqueue on torch's current HIP stream.  Nothing here computes on the CPU.
"""

import ctypes
import logging

import torch

from . import _lib

log = logging.getLogger("func-python-logger")

# The w-stacking NUFFT has two precisions.  epsilon >= 1e-7: fp32 taps and
# uv planes with fp64 coordinates, phases and image accumulation (W <= 8;
# measured on the full C2 workload against the fp64 W = 13 oracle: 9.1e-7
# invert / 8.1e-7 predict relative RMS, tests/test_gpu_fullsize.py).
# epsilon < 1e-7 -- the reference's default 1e-12, which it asks of ducc0
# with double_precision_accumulation (imaging/ng.py:178, :240-256) -- runs
# the fp64 NUFFT (W = ceil(-log10(epsilon/10)) in [9, 16], c128 planes, Z2Z
# FFTs).  precision="fp32" (per call, or set_precision("fp32") for the
# process) keeps such requests on the fp32 path at its floor instead, said so
# once per process.
EPS_FLOOR = 1e-7
_PRECISION = "auto"
_eps_warned = False


def set_precision(mode):
    """Process default for the NUFFT precision: "auto" (fp64 below epsilon
    1e-7) or "fp32" (the fp32 NUFFT at its floor for every epsilon)."""
    global _PRECISION
    if mode not in ("auto", "fp32"):
        raise ValueError("precision must be 'auto' or 'fp32'")
    _PRECISION = mode


def is_fp64(epsilon, precision=None):
    """True when a NUFFT call at `epsilon` runs the fp64 path."""
    mode = precision or _PRECISION
    return float(epsilon) < EPS_FLOOR and mode == "auto"


def _prec_bits(epsilon, precision=None):
    """Flag bits of a NUFFT call for `epsilon` under `precision`."""
    global _eps_warned
    mode = precision or _PRECISION
    if mode not in ("auto", "fp32"):
        raise ValueError("precision must be 'auto' or 'fp32'")
    if float(epsilon) >= EPS_FLOOR or mode == "auto":
        return 0
    if not _eps_warned:
        _eps_warned = True
        log.warning("epsilon %.1e requested with precision='fp32': the HIP w-stacking NUFFT "
                    "runs in fp32 at its floor epsilon %.0e (support W = 8); measured "
                    "dirty-image error vs an fp64 epsilon=1e-12 reference ~1e-6 relative RMS",
                    float(epsilon), EPS_FLOOR)
    return _lib.SDP_HIP_FP32


_DT_CODE = {
    torch.complex64: _lib.SDP_HIP_C64,
    torch.complex128: _lib.SDP_HIP_C128,
    torch.float32: _lib.SDP_HIP_F32,
    torch.float64: _lib.SDP_HIP_F64,
}


def _on_gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a device (HIP) tensor")
    return t


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _alloc(shape, dtype, dev, may_release=True):
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
        release_workspace()
        torch.cuda.empty_cache()
        return torch.empty(shape, dtype=dtype, device=dev)


def _check_wgt(wgt, nrow, nchan):
    """ducc0 takes f64 weights; f32 (the bench's) and f64 are both read in place."""
    if wgt is None:
        return
    _on_gpu(wgt, "wgt")
    if wgt.dtype not in (torch.float32, torch.float64) or tuple(wgt.shape) != (nrow, nchan):
        raise ValueError("wgt must be float32 or float64 [nrow, nchan]")


def _wgt_args(wgt):
    if wgt is None:
        return (_ptr(None), _lib.SDP_HIP_F32, 0, 0)
    return (_ptr(wgt), _DT_CODE[wgt.dtype], wgt.stride(0), wgt.stride(1))


def _check_uvw(uvw):
    _on_gpu(uvw, "uvw")
    if uvw.dtype != torch.float64 or uvw.dim() != 2 or uvw.shape[1] != 3 or uvw.stride(1) != 1:
        raise ValueError("uvw must be float64 [nrow, 3] with unit column stride")


def ms2dirty(uvw, freq, vis, wgt, npix_x, npix_y, pixsize_x, pixsize_y,
             epsilon=1e-7, do_wstacking=True, flip_uw=False, out=None,
             out_strides=None, accumulate=False, precision=None, slot=0):
    """ducc0.wgridder.ms2dirty semantics on device.

    uvw [nrow,3] f64, freq [nchan] f64, vis [nrow,nchan] c64/c128 (or None
    for unit visibilities), wgt [nrow,nchan] f32 (or None).  Returns the
    f64 dirty image [npix_x, npix_y] (or writes ``out`` with
    ``out_strides`` = (stride_x, stride_y) in elements) and an info dict.
    ``slot=1`` uses the library's second scratch set (SDP_HIP_SLOT1): calls
    alternated between two streams and slots overlap on the device.

    ``info["layout_reused"]`` is 1 when the call found the bucketing layout
    its slot kept from the previous invert of the same uvw, freq (by content)
    and geometry, and ran only the value passes of the sort
    (``SDP_HIP_LAYOUT_CACHE=0`` switches the cache off).
    """
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    if vis is not None:
        _on_gpu(vis, "vis")
        if vis.dtype not in (torch.complex64, torch.complex128) or tuple(vis.shape) != (nrow, nchan):
            raise ValueError("vis must be complex [nrow, nchan]")
    _check_wgt(wgt, nrow, nchan)
    if out is None:
        out = _alloc((npix_x, npix_y), torch.float64, dev)
        out_strides = (npix_y, 1)
    elif out_strides is None:
        out_strides = out.stride()
    _on_gpu(out, "out")
    if out.dtype != torch.float64:
        raise ValueError("dirty output must be float64")
    flags = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
             | (_lib.SDP_HIP_SLOT1 if slot else 0) | pbits)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty",
        _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
        _ptr(vis), _DT_CODE[vis.dtype] if vis is not None else _lib.SDP_HIP_C64,
        vis.stride(0) if vis is not None else 0, vis.stride(1) if vis is not None else 0,
        *_wgt_args(wgt),
        int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
        int(bool(do_wstacking)), flags,
        _ptr(out), int(out_strides[0]), int(out_strides[1]),
        _stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def uvw_bounds(uvw, freq):
    """Host {min w, max w, max|u|, max|v|, min f, max f} of device arrays uvw
    [nrow, 3] (metres) and freq: one batch's contribution to the bounds of
    an ms2dirty_batch sequence (combine with merge_bounds)."""
    _check_uvw(uvw)
    b = torch.stack([uvw[:, 2].min(), uvw[:, 2].max(), uvw[:, 0].abs().max(),
                     uvw[:, 1].abs().max(), freq.min().double(), freq.max().double()])
    return [float(x) for x in b.cpu()]


def merge_bounds(*bs):
    return [min(b[0] for b in bs), max(b[1] for b in bs), max(b[2] for b in bs),
            max(b[3] for b in bs), min(b[4] for b in bs), max(b[5] for b in bs)]


def wstack_layout(bounds, npix_x, npix_y, pixsize_x, pixsize_y, epsilon=1e-7, do_wstacking=True,
                  flip_uw=False, precision=None):
    """The w-plane layout an ms2dirty_batch sequence with these ``bounds``
    uses (sdp_hip_wstack_layout, no device work): dict with support, nplanes,
    w0, dw and ``nps`` = the first-plane count a w-slab partition splits."""
    if len(bounds) != 6:
        raise ValueError("bounds: {wmin, wmax, umax, vmax, fmin, fmax}")
    bbuf = (ctypes.c_double * 6)(*[float(x) for x in bounds])
    flags = (_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | _prec_bits(epsilon, precision)
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_wstack_layout", ctypes.cast(bbuf, ctypes.c_void_p), int(npix_x),
              int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
              int(bool(do_wstacking)), flags, ctypes.byref(info))
    d = info.as_dict()
    d["nps"] = d["nplanes"] - d["support"] + 1 if d["nplanes"] > 1 else 1
    return d


def layout_fingerprint(uvw, freq):
    """The content fingerprint an invert keeps its bucketing layout under
    (``info["layout_reused"]``), computed on the host from HOST arrays ``uvw``
    [nrow, 3] and ``freq`` [nchan] (sdp_hip_wstack_fingerprint, no device
    work): four 64-bit words {uvw a, uvw b, freq a, freq b}."""
    import numpy as np
    uvw = np.asarray(uvw, dtype=np.float64)
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    if uvw.ndim != 2 or uvw.shape[1] != 3 or freq.ndim != 1:
        raise ValueError("uvw must be [nrow, 3] and freq [nchan]")
    # (rows with a stride are read in place, as the device arrays are)
    if uvw.strides[1] != 8 or uvw.strides[0] % 8 or uvw.strides[0] < 24:
        uvw = np.ascontiguousarray(uvw)
    out = (ctypes.c_uint64 * 4)()
    _lib.call("sdp_hip_wstack_fingerprint", ctypes.c_void_p(uvw.ctypes.data),
              uvw.strides[0] // 8, uvw.shape[0],
              ctypes.c_void_p(freq.ctypes.data), freq.shape[0], ctypes.cast(out, ctypes.c_void_p))
    return tuple(int(x) for x in out)


def ms2dirty_batch(uvw, freq, vis, wgt, npix_x, npix_y, pixsize_x, pixsize_y, bounds,
                   first, last, epsilon=1e-7, do_wstacking=True, flip_uw=False, out=None,
                   out_strides=None, accumulate=False, precision=None, slab=None):
    """One batch of a batched invert (sdp_hip_ms2dirty_batch): the batch is
    gridded into the resident w planes shared by the whole sequence; the
    ``first`` batch zeroes them, the ``last`` runs the FFT and w-screens into
    ``out`` (allocated if None; earlier batches return None).  ``bounds``:
    merge_bounds over every batch of the sequence.  ``slab`` = (lo, hi): grid
    only the visibilities whose first w plane of the sequence's layout
    (wstack_layout) lies in [lo, hi), into that slab's planes only
    (SDP_HIP_W_SLAB; the slabs of one layout sum to the full image)."""
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    if vis is not None:
        _on_gpu(vis, "vis")
        if vis.dtype not in (torch.complex64, torch.complex128) or tuple(vis.shape) != (nrow, nchan):
            raise ValueError("vis must be complex [nrow, nchan]")
    _check_wgt(wgt, nrow, nchan)
    if last:
        if out is None:
            # (never auto-release the workspace here: past the first batch it
            # holds the sequence's resident planes)
            out = _alloc((npix_x, npix_y), torch.float64, dev, may_release=first)
            out_strides = (npix_y, 1)
        elif out_strides is None:
            out_strides = out.stride()
        _on_gpu(out, "out")
        if out.dtype != torch.float64:
            raise ValueError("dirty output must be float64")
    if len(bounds) != 6:
        raise ValueError("bounds: {wmin, wmax, umax, vmax, fmin, fmax}")
    vals = [float(x) for x in bounds]
    if slab is not None:
        lo, hi = (int(x) for x in slab)
        if not 0 <= lo < hi:
            raise ValueError("slab: first planes (lo, hi) with 0 <= lo < hi")
        vals += [float(lo), float(hi)]
    bbuf = (ctypes.c_double * len(vals))(*vals)
    flags = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
             | (_lib.SDP_HIP_BATCH_FIRST if first else 0) | (_lib.SDP_HIP_BATCH_LAST if last else 0)
             | (_lib.SDP_HIP_W_SLAB if slab is not None else 0) | pbits)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty_batch",
        _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
        _ptr(vis), _DT_CODE[vis.dtype] if vis is not None else _lib.SDP_HIP_C64,
        vis.stride(0) if vis is not None else 0, vis.stride(1) if vis is not None else 0,
        *_wgt_args(wgt),
        int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
        int(bool(do_wstacking)), flags, ctypes.cast(bbuf, ctypes.c_void_p),
        _ptr(out if last else None), int(out_strides[0]) if last else 0,
        int(out_strides[1]) if last else 0, _stream(dev), ctypes.byref(info))
    return (out if last else None), info.as_dict()


def _host3(v):
    """(l, m, n-1) as a host double[3] for the C ABI, or NULL."""
    if v is None:
        return None
    return ctypes.cast((ctypes.c_double * 3)(*[float(x) for x in v]), ctypes.c_void_p)


_FLAG_DT = {torch.int64: 8, torch.int32: 4, torch.int8: 1, torch.uint8: 1, torch.bool: 1}


def ms2dirty_vis(uvw, freq, vis, pol, wgt, flags, coef, npix_x, npix_y, pixsize_x, pixsize_y,
                 epsilon=1e-7, do_wstacking=True, flip_uw=False, out=None, out_strides=None,
                 accumulate=False, sumwt=None, shift_lmn=None, keep_buckets=False,
                 reuse_buckets=False, precision=None, slot=0, bounds=None, first=False,
                 last=False):
    """ms2dirty with invert_ng's visibility prologue fused in
    (sdp_hip_ms2dirty_vis): ``vis`` [nrow, nchan, npol_vis] complex (any
    strides, read in place; None = unit visibilities), ``flags`` the same
    shape (integer / bool, or None), ``wgt`` [nrow, nchan] f32/f64 weights of
    image pol ``pol``, ``coef`` the conversion-matrix row for that pol
    (complex [npol_vis]) or None for no conversion, ``sumwt`` a one-element
    f64 device view that receives += the masked weight sum.

    ``keep_buckets`` buckets every in-grid visibility and keeps the bucketing
    on the device; a following call with ``reuse_buckets`` and the same uvw,
    freq and geometry (another image pol) runs only the value pass, gridding
    and FFT (SDP_HIP_KEEP_BUCKETS / SDP_HIP_REUSE_BUCKETS).  ``slot=1`` uses
    the library's second scratch set (SDP_HIP_SLOT1; not with kept / reused
    buckets): calls alternated between two streams and slots overlap.

    ``bounds`` (uvw_bounds / merge_bounds of the whole sequence) makes the
    call one batch of a sequence sharing one set of resident w planes
    (sdp_hip_ms2dirty_vis_batch, as ms2dirty_batch): ``first`` zeroes them,
    ``last`` transforms them into ``out``."""
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    npv = 1
    if vis is not None:
        _on_gpu(vis, "vis")
        if vis.dtype not in (torch.complex64, torch.complex128) or vis.dim() != 3 or \
                tuple(vis.shape[:2]) != (nrow, nchan):
            raise ValueError("vis must be complex [nrow, nchan, npol]")
        npv = vis.shape[2]
    if flags is not None:
        _on_gpu(flags, "flags")
        if flags.dtype not in _FLAG_DT or flags.dim() != 3 or tuple(flags.shape[:2]) != (nrow, nchan):
            raise ValueError("flags must be an integer [nrow, nchan, npol] tensor")
        npv = max(npv, flags.shape[2])
    if wgt is not None:
        _on_gpu(wgt, "wgt")
        if wgt.dtype not in (torch.float32, torch.float64) or tuple(wgt.shape) != (nrow, nchan):
            raise ValueError("wgt must be float32/float64 [nrow, nchan]")
    if not 0 <= pol < npv:
        raise ValueError("pol out of range")
    cbuf = None
    if coef is not None:
        c = [complex(x) for x in coef]
        if len(c) != npv:
            raise ValueError("coef must have one entry per visibility pol")
        cbuf = (ctypes.c_double * (2 * npv))(*[v for z in c for v in (z.real, z.imag)])
    if out is None:
        out = _alloc((npix_x, npix_y), torch.float64, dev)
        out_strides = (npix_y, 1)
    elif out_strides is None:
        out_strides = out.stride()
    _on_gpu(out, "out")
    if out.dtype != torch.float64:
        raise ValueError("dirty output must be float64")
    if sumwt is not None and (sumwt.dtype != torch.float64 or not sumwt.is_cuda):
        raise ValueError("sumwt must be a float64 device tensor")
    bits = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
            | pbits)
    bits |= (_lib.SDP_HIP_KEEP_BUCKETS if keep_buckets else 0) | \
        (_lib.SDP_HIP_REUSE_BUCKETS if reuse_buckets else 0) | (_lib.SDP_HIP_SLOT1 if slot else 0)
    info = _lib.WGridInfo()
    batch = ()
    name = "sdp_hip_ms2dirty_vis"
    if bounds is not None:
        if len(bounds) != 6:
            raise ValueError("bounds: {wmin, wmax, umax, vmax, fmin, fmax}")
        bits |= (_lib.SDP_HIP_BATCH_FIRST if first else 0) | (_lib.SDP_HIP_BATCH_LAST if last else 0)
        bbuf = (ctypes.c_double * 6)(*[float(x) for x in bounds])
        batch = (ctypes.cast(bbuf, ctypes.c_void_p),)
        name = "sdp_hip_ms2dirty_vis_batch"
    _lib.call(
        name,
        _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
        _ptr(vis), _DT_CODE[vis.dtype] if vis is not None else _lib.SDP_HIP_C64,
        *(vis.stride() if vis is not None else (0, 0, 0)), npv,
        ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None,
        _ptr(wgt), _DT_CODE[wgt.dtype] if wgt is not None else _lib.SDP_HIP_F32,
        *(wgt.stride() if wgt is not None else (0, 0)),
        _ptr(flags), _FLAG_DT[flags.dtype] if flags is not None else 0,
        *(flags.stride() if flags is not None else (0, 0, 0)), int(pol),
        int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
        int(bool(do_wstacking)), bits, *batch,
        _ptr(out), int(out_strides[0]), int(out_strides[1]), _ptr(sumwt), _host3(shift_lmn),
        _stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def ms2dirty_vis_pols(uvw, freq, vis, wgt, flags, coef, npix_x, npix_y, pixsize_x, pixsize_y,
                      epsilon=1e-7, do_wstacking=True, flip_uw=False, out=None, out_strides=None,
                      accumulate=False, sumwt=None, shift_lmn=None, precision=None):
    """Every image pol of one invert_ng image channel in one call
    (sdp_hip_ms2dirty_vis_pols): ``vis`` [nrow, nchan, npol_vis] complex and
    ``flags`` (integer, or None) as ms2dirty_vis, ``wgt`` [nrow, nchan,
    >= npol_img] f32/f64 (image pol q takes the weights and flags of pol q),
    ``coef`` the conversion matrix [npol_img, npol_vis] (complex) or None for
    the identity.  ``out`` [npol_img, ...] f64 with ``out_strides`` = (pol,
    x, y) element strides; ``sumwt`` a [npol_img] f64 device view (+= each
    pol's masked weight sum).  The pols share one bucketing and one value
    pass; results as one ms2dirty_vis call per image pol."""
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    _on_gpu(vis, "vis")
    if vis.dtype not in (torch.complex64, torch.complex128) or vis.dim() != 3 or \
            tuple(vis.shape[:2]) != (nrow, nchan):
        raise ValueError("vis must be complex [nrow, nchan, npol]")
    npv = vis.shape[2]
    if flags is not None:
        _on_gpu(flags, "flags")
        if flags.dtype not in _FLAG_DT or tuple(flags.shape) != tuple(vis.shape):
            raise ValueError("flags must be an integer tensor shaped as vis")
    _on_gpu(wgt, "wgt")
    if wgt.dtype not in (torch.float32, torch.float64) or wgt.dim() != 3 or \
            tuple(wgt.shape[:2]) != (nrow, nchan):
        raise ValueError("wgt must be float32/float64 [nrow, nchan, npol]")
    npo = npv if coef is None else len(coef)
    if not 1 <= npo <= min(npv, wgt.shape[2]):
        raise ValueError("npol_img must be 1..npol_vis (and have weights)")
    cbuf = None
    if coef is not None:
        rows = [[complex(z) for z in r] for r in coef]
        if any(len(r) != npv for r in rows):
            raise ValueError("coef rows must have one entry per visibility pol")
        cbuf = (ctypes.c_double * (2 * npo * npv))(
            *[v for r in rows for z in r for v in (z.real, z.imag)])
    if out is None:
        out = _alloc((npo, npix_x, npix_y), torch.float64, dev)
        out_strides = out.stride()
    elif out_strides is None:
        out_strides = out.stride()
    _on_gpu(out, "out")
    if out.dtype != torch.float64:
        raise ValueError("dirty output must be float64")
    if sumwt is not None and (sumwt.dtype != torch.float64 or not sumwt.is_cuda or
                              sumwt.numel() < npo):
        raise ValueError("sumwt must be a float64 device tensor with one entry per image pol")
    bits = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
            | pbits)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty_vis_pols",
        _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
        _ptr(vis), _DT_CODE[vis.dtype], *vis.stride(), npv,
        ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None, npo,
        _ptr(wgt), _DT_CODE[wgt.dtype], *wgt.stride(),
        _ptr(flags), _FLAG_DT[flags.dtype] if flags is not None else 0,
        *(flags.stride() if flags is not None else (0, 0, 0)),
        int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
        int(bool(do_wstacking)), bits,
        _ptr(out), int(out_strides[1]), int(out_strides[2]), int(out_strides[0]),
        _ptr(sumwt), int(sumwt.stride(0)) if sumwt is not None else 0, _host3(shift_lmn),
        _stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def dirty2ms_vis(uvw, freq, dirty, out, coef, pixsize_x, pixsize_y, epsilon=1e-7,
                 do_wstacking=True, flip_uw=False, dirty_strides=None, npix=None,
                 accumulate=False, shift_lmn=None, precision=None):
    """One image pol of predict_ng with the pol conversion fused into the
    write-back (sdp_hip_dirty2ms_vis): ``out`` [nrow, nchan, npol_vis] complex
    (any strides) gets coef[k] * predicted vis in pol k (coef None: pol 0)."""
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    _on_gpu(dirty, "dirty")
    if dirty.dtype != torch.float64:
        raise ValueError("dirty must be float64")
    npix_x, npix_y = (dirty.shape[-2], dirty.shape[-1]) if npix is None else npix
    if dirty_strides is None:
        dirty_strides = dirty.stride()[-2:]
    _on_gpu(out, "out")
    if out.dtype not in (torch.complex64, torch.complex128) or out.dim() != 3 or \
            tuple(out.shape[:2]) != (nrow, nchan):
        raise ValueError("out must be complex [nrow, nchan, npol]")
    npv = out.shape[2]
    cbuf = None
    if coef is not None:
        c = [complex(x) for x in coef]
        if len(c) != npv:
            raise ValueError("coef must have one entry per visibility pol")
        cbuf = (ctypes.c_double * (2 * npv))(*[v for z in c for v in (z.real, z.imag)])
    bits = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
            | pbits)
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_dirty2ms_vis", _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
              _ptr(dirty), int(dirty_strides[0]), int(dirty_strides[1]), int(npix_x), int(npix_y),
              float(pixsize_x), float(pixsize_y), float(epsilon), int(bool(do_wstacking)), bits,
              _ptr(out), _DT_CODE[out.dtype], *out.stride(), npv,
              ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None,
              _host3(shift_lmn), _stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def dirty2ms_vis_pols(uvw, freq, dirty, out, coef, pixsize_x, pixsize_y, epsilon=1e-7,
                      do_wstacking=True, flip_uw=False, dirty_strides=None, npix=None,
                      accumulate=False, shift_lmn=None, precision=None):
    """Every image pol of predict_ng in one call (sdp_hip_dirty2ms_vis_pols):
    ``dirty`` [npol_img, ...] f64 with ``dirty_strides`` = (pol, x, y),
    ``out`` [nrow, nchan, npol_vis] complex (any strides) gets
    sum_q coef[q][k] * prediction_q in vis pol k (coef None: identity).  The
    pols share one bucketing and one write-back; results as one dirty2ms_vis
    call per image pol, accumulating after the first."""
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    _on_gpu(dirty, "dirty")
    if dirty.dtype != torch.float64 or dirty.dim() != 3:
        raise ValueError("dirty must be float64 [npol_img, nx, ny]")
    npo = dirty.shape[0]
    npix_x, npix_y = (dirty.shape[-2], dirty.shape[-1]) if npix is None else npix
    if dirty_strides is None:
        dirty_strides = dirty.stride()
    _on_gpu(out, "out")
    if out.dtype not in (torch.complex64, torch.complex128) or out.dim() != 3 or \
            tuple(out.shape[:2]) != (nrow, nchan):
        raise ValueError("out must be complex [nrow, nchan, npol]")
    npv = out.shape[2]
    if not 1 <= npo <= 4:
        raise ValueError("npol_img must be 1..4")
    cbuf = None
    if coef is not None:
        rows = [[complex(z) for z in r] for r in coef]
        if len(rows) != npo or any(len(r) != npv for r in rows):
            raise ValueError("coef must be [npol_img][npol_vis]")
        cbuf = (ctypes.c_double * (2 * npo * npv))(
            *[v for r in rows for z in r for v in (z.real, z.imag)])
    bits = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
            | pbits)
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_dirty2ms_vis_pols", _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
              _ptr(dirty), int(dirty_strides[1]), int(dirty_strides[2]), int(dirty_strides[0]),
              npo, int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
              int(bool(do_wstacking)), bits, _ptr(out), _DT_CODE[out.dtype], *out.stride(), npv,
              ctypes.cast(cbuf, ctypes.c_void_p) if cbuf is not None else None,
              _host3(shift_lmn), _stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def dirty2ms(uvw, freq, dirty, wgt, pixsize_x, pixsize_y, epsilon=1e-7,
             do_wstacking=True, flip_uw=False, out=None, dirty_strides=None,
             npix=None, accumulate=False, vis_dtype=torch.complex64, precision=None):
    """ducc0.wgridder.dirty2ms semantics on device; returns vis [nrow,nchan]."""
    pbits = _prec_bits(epsilon, precision)
    _check_uvw(uvw)
    dev = uvw.device
    freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
    nrow, nchan = uvw.shape[0], freq.shape[0]
    _on_gpu(dirty, "dirty")
    if dirty.dtype != torch.float64:
        raise ValueError("dirty must be float64")
    if npix is None:
        npix_x, npix_y = dirty.shape[-2], dirty.shape[-1]
    else:
        npix_x, npix_y = npix
    if dirty_strides is None:
        dirty_strides = dirty.stride()[-2:]
    _check_wgt(wgt, nrow, nchan)
    if out is None:
        out = _alloc((nrow, nchan), vis_dtype, dev)
    _on_gpu(out, "vis out")
    if out.dtype not in (torch.complex64, torch.complex128) or tuple(out.shape) != (nrow, nchan):
        raise ValueError("vis out must be complex [nrow, nchan]")
    flags = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
             | pbits)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_dirty2ms",
        _ptr(uvw), uvw.stride(0), _ptr(freq), nchan, nrow,
        _ptr(dirty), int(dirty_strides[0]), int(dirty_strides[1]), int(npix_x), int(npix_y),
        float(pixsize_x), float(pixsize_y),
        *_wgt_args(wgt),
        float(epsilon), int(bool(do_wstacking)), flags,
        _ptr(out), _DT_CODE[out.dtype], out.stride(0), out.stride(1),
        _stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def set_stage_timing(enable):
    _lib.load().sdp_hip_set_stage_timing(int(bool(enable)))


def release_workspace():
    _lib.call("sdp_hip_release_workspace")


def dft_point(direction_cosines, fluxes, uvw, freq=None, out=None, vis_dtype=torch.complex64):
    """Sky-component DFT on device.

    direction_cosines [ncomp,3] f64, fluxes [ncomp, 1|nchan, npol] c128.
    With ``freq`` given, ``uvw`` is [nrow,3] metres (lambda scaling fused);
    otherwise ``uvw`` is uvw_lambda [nrow, nchan, 3] (dft_point_v00 layout).
    Returns vis [nrow, nchan, npol].
    """
    dc = _on_gpu(direction_cosines, "direction_cosines").to(torch.float64).contiguous()
    fl = _on_gpu(fluxes, "fluxes").to(torch.complex128).contiguous()
    if fl.dim() != 3 or dc.dim() != 2 or dc.shape[1] != 3 or fl.shape[0] != dc.shape[0]:
        raise ValueError("direction_cosines [ncomp,3] and fluxes [ncomp,nchan,npol] required")
    ncomp, fnchan, npol = fl.shape
    uvw = _on_gpu(uvw, "uvw").to(torch.float64).contiguous()
    if freq is not None:
        freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
        nrow, nchan = uvw.shape[0], freq.shape[0]
    else:
        nrow, nchan = uvw.shape[0], uvw.shape[1]
    if out is None:
        out = _alloc((nrow, nchan, npol), vis_dtype, uvw.device)
    if not out.is_contiguous() or tuple(out.shape) != (nrow, nchan, npol):
        raise ValueError("vis out must be contiguous [nrow, nchan, npol]")
    if freq is not None:
        _lib.call("sdp_hip_dft_point_metres", ncomp, _ptr(dc), _ptr(fl), fnchan, npol, nrow, nchan,
                  _ptr(uvw), _ptr(freq), _ptr(out), _DT_CODE[out.dtype], _stream(uvw.device))
    else:
        _lib.call("sdp_hip_dft_point_v00", ncomp, _ptr(dc), _ptr(fl), fnchan, npol, nrow, nchan,
                  _ptr(uvw), _ptr(out), _DT_CODE[out.dtype], _stream(uvw.device))
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
    dc = _on_gpu(direction_cosines, "direction_cosines").to(torch.float64).contiguous()
    if dc.dim() != 2 or dc.shape[1] != 3:
        raise ValueError("direction_cosines [ncomp,3] required")
    vis = _on_gpu(vis, "vis")
    if vis.dtype not in (torch.complex64, torch.complex128) or vis.dim() != 3:
        raise ValueError("vis must be complex64 or complex128 [nrow, nchan, npol]")
    vis = vis.contiguous()
    nrow, nchan, npol = vis.shape
    weight = _on_gpu(weight, "weight").to(torch.float64).contiguous()
    if tuple(weight.shape) != (nrow, nchan, npol):
        raise ValueError("weight must be shaped like vis")
    fb = 0
    if flags is not None:
        flags = _on_gpu(flags, "flags").contiguous()
        if tuple(flags.shape) != (nrow, nchan, npol) or flags.dtype not in _FLAG_DT:
            raise ValueError("flags must be an integer tensor shaped like vis")
        fb = _FLAG_DT[flags.dtype]
    uvw = _on_gpu(uvw, "uvw").to(torch.float64).contiguous()
    if freq is not None:
        freq = _on_gpu(freq, "freq").to(torch.float64).contiguous()
        if tuple(uvw.shape) != (nrow, 3) or tuple(freq.shape) != (nchan,):
            raise ValueError("uvw [nrow,3] metres and freq [nchan] must match vis")
    elif tuple(uvw.shape) != (nrow, nchan, 3):
        raise ValueError("uvw_lambda [nrow, nchan, 3] must match vis")
    ncomp = dc.shape[0]
    if out is None:
        out = (_alloc((ncomp, nchan, npol), torch.complex128, vis.device),
               _alloc((nchan, npol), torch.float64, vis.device))
    flux_sum, sumwt = out
    if (not flux_sum.is_contiguous() or tuple(flux_sum.shape) != (ncomp, nchan, npol)
            or flux_sum.dtype != torch.complex128 or not sumwt.is_contiguous()
            or tuple(sumwt.shape) != (nchan, npol) or sumwt.dtype != torch.float64):
        raise ValueError("out must be contiguous (flux_sum [ncomp, nchan, npol] complex128, "
                         "sumwt [nchan, npol] float64)")
    if freq is not None:
        _lib.call("sdp_hip_idft_point_metres", ncomp, _ptr(dc), npol, nrow, nchan, _ptr(uvw),
                  _ptr(freq), _ptr(vis), _DT_CODE[vis.dtype], _ptr(weight), _ptr(flags), fb,
                  _ptr(flux_sum), _ptr(sumwt), _stream(vis.device))
    else:
        _lib.call("sdp_hip_idft_point_v00", ncomp, _ptr(dc), npol, nrow, nchan, _ptr(uvw),
                  _ptr(vis), _DT_CODE[vis.dtype], _ptr(weight), _ptr(flags), fb,
                  _ptr(flux_sum), _ptr(sumwt), _stream(vis.device))
    return flux_sum, sumwt


def canonical_baselines(ant1, ant2, nants):
    """Canonical (a1 < a2) CSR order of a baseline list.

    Returns (perm, conj, row_start, ant2_sorted): ``perm[k]`` is the input
    baseline placed at canonical position k, ``conj[k]`` is True when it was
    given as (a2, a1) (its value must be conjugated), and autocorrelations
    (a1 == a2, zeroed by the reference solver, solvers.py:251-253) are dropped.
    """
    import numpy as np
    a1 = np.asarray(ant1, dtype=np.int64)
    a2 = np.asarray(ant2, dtype=np.int64)
    keep = np.nonzero(a1 != a2)[0]
    lo = np.minimum(a1[keep], a2[keep])
    hi = np.maximum(a1[keep], a2[keep])
    order = np.lexsort((hi, lo))
    perm = keep[order]
    conj = (a1[perm] > a2[perm])
    lo, hi = lo[order], hi[order]
    row_start = np.zeros(nants + 1, dtype=np.int32)
    np.add.at(row_start, lo + 1, 1)
    row_start = np.cumsum(row_start).astype(np.int32)
    return perm, conj, row_start, hi.astype(np.int32)


def solve_gains(xb, wb, gain, gwt, row_start, ant2, mode, niter=200, tol=1e-6,
                phase_only=True, refant=0, damping=0.5):
    """Batched StefCal on device.

    xb [nsolve, nbl, nchan, npol] c128, wb [...] f64 in canonical baseline
    order; gain/gwt [nsolve, nants, nchan, nrec, nrec] (c128 / f64) updated
    in place.  Returns (residual [nsolve, nchan, nrec, nrec], niter_used).
    """
    xb = _on_gpu(xb, "xb").to(torch.complex128).contiguous()
    wb = _on_gpu(wb, "wb").to(torch.float64).contiguous()
    if not (gain.is_cuda and gain.dtype == torch.complex128 and gain.is_contiguous()):
        raise ValueError("gain must be a contiguous complex128 device tensor")
    if not (gwt.is_cuda and gwt.dtype == torch.float64 and gwt.is_contiguous()):
        raise ValueError("gwt must be a contiguous float64 device tensor")
    nsolve, nbl, nchan, npol = xb.shape
    nants = gain.shape[1]
    nrec = gain.shape[3]
    rs = torch.as_tensor(row_start, dtype=torch.int32, device=xb.device)
    a2 = torch.as_tensor(ant2, dtype=torch.int32, device=xb.device)
    residual = torch.zeros((nsolve, nchan, nrec, nrec), dtype=torch.float64, device=xb.device)
    used = torch.zeros(nsolve, dtype=torch.int32, device=xb.device)
    _lib.call("sdp_hip_solve_gains", nsolve, nants, nbl, _ptr(rs), _ptr(a2), nchan, npol,
              int(mode), _ptr(xb), _ptr(wb), _ptr(gain), _ptr(gwt), _ptr(residual), _ptr(used),
              int(niter), float(tol), int(bool(phase_only)), int(refant), float(damping),
              _stream(xb.device))
    return residual, used


def _check_cf_operands(maps, vis_to_im, cf, grid, nrow, nchan, npol):
    """Operand checks shared by grid_cf / degrid_cf: dtypes, contiguity,
    shapes, and the image channel of every visibility channel.  The
    reference indexes ``gd[imchan]`` / ``cf[imchan]`` with numpy
    (grid_data/gridding.py:226-245, :560-580): an index past the GridData's
    (or the CF's) channel axis raises IndexError and a negative one counts
    from the end, so vis_to_im is checked here and negatives are wrapped.
    Returns the (possibly wrapped) int32 vis_to_im on the device."""
    cfn, cf_npol, _, _, _, gv, gu = cf.shape
    gn, g_npol, ny, nx = grid.shape
    if cf.dtype != torch.complex128 or grid.dtype != torch.complex128:
        raise ValueError("cf and grid must be complex128")
    if not (cf.is_contiguous() and grid.is_contiguous()):
        raise ValueError("cf and grid must be contiguous")
    if cf_npol != npol or g_npol != npol:
        raise ValueError(f"pol axes differ: vis {npol}, cf {cf_npol}, grid {g_npol}")
    for k in ("pu", "pv", "pwc", "pdu", "pdv"):
        m = maps[k]
        if m.dtype != torch.int32 or not m.is_contiguous() or tuple(m.shape) != (nchan, nrow):
            raise ValueError(f"map {k} must be contiguous int32 [{nchan}, {nrow}]")
    v2i = vis_to_im.detach().to("cpu", torch.int64)
    if v2i.numel() != nchan:
        raise ValueError(f"vis_to_im has {v2i.numel()} entries for {nchan} channels")
    lim = min(gn, cfn)
    if bool((v2i >= lim).any()) or bool((v2i < -lim).any()):
        raise IndexError(f"vis_to_im {v2i.tolist()} out of range for {gn} grid / {cfn} cf "
                         "channels")
    if bool((v2i < 0).any()):
        # numpy wraps gd[imchan] by the grid's channel count and cf[imchan] by
        # the CF's: one kernel index serves both only when the counts agree
        if gn != cfn:
            raise IndexError(f"negative vis_to_im {v2i.tolist()} with {gn} grid and {cfn} cf "
                             "channels: the reference would pick different grid and cf "
                             "channels; pass non-negative channel indices")
        v2i = torch.where(v2i < 0, v2i + gn, v2i)
    return v2i.to(device=grid.device, dtype=torch.int32)


def grid_cf(maps, vis_to_im, vis, wt, cf, grid, sumwt):
    """Convolution-function gridding (accumulates into grid and sumwt).

    maps: dict of int32 [nchan, nrow] device tensors pu, pv, pwc, pdu, pdv;
    vis [nrow, nchan, npol] c128, wt f64 same shape; cf [c, p, nw, ndv, ndu,
    gv, gu] c128; grid [g_nchan, npol, ny, nx] c128; sumwt [g_nchan, npol] f64.
    Returns the number of skipped (row, pol) samples.
    """
    nrow, nchan, npol = vis.shape
    cfn, _, nw, ndv, ndu, gv, gu = cf.shape
    gn, _, ny, nx = grid.shape
    if vis.dtype != torch.complex128 or wt.dtype != torch.float64 or sumwt.dtype != torch.float64:
        raise ValueError("grid_cf: vis complex128, wt and sumwt float64")
    if tuple(wt.shape) != (nrow, nchan, npol) or tuple(sumwt.shape) != (gn, npol):
        raise ValueError("grid_cf: wt must match vis, sumwt must be [g_nchan, npol]")
    for t in (vis, wt, sumwt):
        if not t.is_contiguous():
            raise ValueError("grid_cf operands must be contiguous")
    v2i = _check_cf_operands(maps, vis_to_im, cf, grid, nrow, nchan, npol)
    skipped = torch.zeros(1, dtype=torch.int64, device=vis.device)
    _lib.call("sdp_hip_grid_cf", nrow, nchan, npol, _ptr(maps["pu"]), _ptr(maps["pv"]),
              _ptr(maps["pwc"]), _ptr(maps["pdu"]), _ptr(maps["pdv"]), _ptr(v2i), _ptr(vis),
              _ptr(wt), _ptr(cf), cfn, nw, ndv, ndu, gv, gu, _ptr(grid), gn, ny, nx, _ptr(sumwt),
              _ptr(skipped), _stream(vis.device))
    return skipped


def degrid_cf(maps, vis_to_im, grid, cf, nrow, nchan, out):
    """Convolution-function degridding into out [nrow, nchan, npol] c128
    (skipped samples are written as zero).  Returns the skipped count."""
    cfn, npol, nw, ndv, ndu, gv, gu = cf.shape
    gn, _, ny, nx = grid.shape
    if out.dtype != torch.complex128 or not out.is_contiguous() or \
            tuple(out.shape) != (nrow, nchan, npol):
        raise ValueError(f"degrid_cf: out must be contiguous complex128 [{nrow}, {nchan}, {npol}]")
    v2i = _check_cf_operands(maps, vis_to_im, cf, grid, nrow, nchan, npol)
    skipped = torch.zeros(1, dtype=torch.int64, device=grid.device)
    _lib.call("sdp_hip_degrid_cf", nrow, nchan, npol, _ptr(maps["pu"]), _ptr(maps["pv"]),
              _ptr(maps["pwc"]), _ptr(maps["pdu"]), _ptr(maps["pdv"]), _ptr(v2i),
              _ptr(grid), gn, ny, nx, _ptr(cf), cfn, nw, ndv, ndu, gv, gu, _ptr(out),
              _ptr(skipped), _stream(grid.device))
    return skipped


# ---- imaging weights (sdp_hip_grid_weights / sdp_hip_reweight / sdp_hip_taper)
_FLAG_BYTES = {torch.int64: 8, torch.int32: 4, torch.int8: 1, torch.uint8: 1, torch.bool: 1}
WEIGHTING = {"natural": 0, "uniform": 1, "robust": 2}


def _weight_operands(uvw, freq, weight, flags):
    _check_uvw(uvw)
    for t, n in ((freq, "freq"), (weight, "weight")):
        _on_gpu(t, n)
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{n} must be a contiguous float64 device tensor")
    if not uvw.is_contiguous():
        raise ValueError("uvw must be contiguous [nrow, 3]")
    nrow, nchan, npol = weight.shape
    if uvw.shape[0] != nrow or freq.numel() != nchan:
        raise ValueError("weight must be [nrow, nchan, npol] matching uvw and freq")
    fb = 0
    if flags is not None:
        _on_gpu(flags, "flags")
        if flags.shape != weight.shape or not flags.is_contiguous() or flags.dtype not in _FLAG_BYTES:
            raise ValueError("flags must be a contiguous integer tensor shaped like weight")
        fb = _FLAG_BYTES[flags.dtype]
    return nrow, nchan, npol, fb


def _wcs6(wcs):
    return torch.tensor([float(x) for ax in wcs for x in ax], dtype=torch.float64)


def grid_weights(uvw, freq, weight, flags, vis_to_im, wcs, grid, sumwt):
    """Accumulate flagged weights into ``grid`` [g_nchan, npol, ny, nx] f64 and
    ``sumwt`` [g_nchan, npol]; ``wcs`` = ((crval, cdelt, crpix) of UU, of VV).
    Returns the device count of skipped (row, chan, pol) samples."""
    nrow, nchan, npol, fb = _weight_operands(uvw, freq, weight, flags)
    gn, gp, ny, nx = grid.shape
    if gp != npol or grid.dtype != torch.float64 or not grid.is_contiguous():
        raise ValueError("grid must be contiguous float64 [g_nchan, npol, ny, nx]")
    if sumwt.shape != (gn, npol) or sumwt.dtype != torch.float64:
        raise ValueError("sumwt must be float64 [g_nchan, npol]")
    w6 = _wcs6(wcs).to(uvw.device)
    skipped = torch.zeros(1, dtype=torch.int64, device=uvw.device)
    _lib.call("sdp_hip_grid_weights", nrow, nchan, npol, _ptr(uvw), _ptr(freq), _ptr(weight),
              _ptr(flags), fb, _ptr(vis_to_im), _ptr(w6), _ptr(grid), gn, ny, nx, _ptr(sumwt),
              _ptr(skipped), _stream(uvw.device))
    return skipped


def reweight(uvw, freq, weight, flags, vis_to_im, wcs, grid, imaging_weight, weighting="uniform",
             robustness=0.0, sumwt=None):
    """Overwrite ``imaging_weight`` [nrow, nchan, npol] f64 in place."""
    if weighting not in WEIGHTING:
        raise AssertionError(f"Weighting {weighting} not supported")
    nrow, nchan, npol, fb = _weight_operands(uvw, freq, weight, flags)
    _on_gpu(imaging_weight, "imaging_weight")
    if (imaging_weight.shape != weight.shape or imaging_weight.dtype != torch.float64
            or not imaging_weight.is_contiguous()):
        raise ValueError("imaging_weight must be contiguous float64 shaped like weight")
    coef = (5.0 * 10.0 ** (-robustness)) ** 2
    if grid is None:
        gn, ny, nx, w6 = 1, 1, 1, torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0, 1.0], dtype=torch.float64)
    else:
        gn, _, ny, nx = grid.shape
        w6 = _wcs6(wcs)
    w6 = w6.to(uvw.device)
    ns = 0 if sumwt is None else sumwt.numel()
    _lib.call("sdp_hip_reweight", nrow, nchan, npol, _ptr(uvw), _ptr(freq), _ptr(weight),
              _ptr(flags), fb, _ptr(vis_to_im), _ptr(w6), _ptr(grid), gn, ny, nx,
              WEIGHTING[weighting], coef, _ptr(sumwt), ns, _ptr(imaging_weight),
              _stream(uvw.device))
    return imaging_weight


def taper(uvw, freq, flags, imaging_weight, kind, param):
    """In place: imaging_weight = flagged imaging weight * taper; kind
    "gaussian" (param = pi^2 beam^2 / (4 ln 2)) or "tukey" (param = r)."""
    nrow, nchan, npol, fb = _weight_operands(uvw, freq, imaging_weight, flags)
    _lib.call("sdp_hip_taper", nrow, nchan, npol, _ptr(uvw), _ptr(freq), _ptr(flags), fb,
              {"gaussian": 0, "tukey": 1}[kind], float(param), _ptr(imaging_weight),
              _stream(uvw.device))
    return imaging_weight


# ---- calibration neighbours (sdp_hip_point_sums / divide_vis / apply_gains)
def _vis4(t, name):
    _on_gpu(t, name)
    if t.dtype not in (torch.complex64, torch.complex128) or t.dim() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous complex [t, b, f, p] tensor")
    return t


def _flags_of(flags, shape):
    if flags is None:
        return None, 0
    _on_gpu(flags, "flags")
    if tuple(flags.shape) != tuple(shape) or not flags.is_contiguous() or flags.dtype not in _FLAG_DT:
        raise ValueError("flags must be a contiguous integer tensor shaped like vis")
    return flags, _FLAG_DT[flags.dtype]


def point_sums(vis, model, weight, flags, row_ptr, time_idx, nchan_g, perm=None, conj=None,
               model_flags=None):
    """x_b, xwt_b [nrow_g, nbl, nchan_g, npol] (c128, f64) of solve_gaintable
    over divide_visibility(vis, model) (model None: vis itself)."""
    _vis4(vis, "vis")
    if model is not None:
        _vis4(model, "model")
        if model.shape != vis.shape or model.dtype != vis.dtype:
            raise ValueError("model must match vis")
    nt, nbl, nchan, npol = vis.shape
    if weight is not None and (weight.shape != vis.shape or weight.dtype != torch.float64
                               or not weight.is_contiguous()):
        raise ValueError("weight must be contiguous float64 shaped like vis")
    fl, fb = _flags_of(flags, vis.shape)
    nrow_g = row_ptr.numel() - 1
    nout = nbl if perm is None else perm.numel()
    if perm is not None and (perm.dtype != torch.int32 or (conj is not None and (
            conj.dtype != torch.uint8 or conj.numel() != nout))):
        raise ValueError("perm must be int32 and conj uint8 of the same length")
    xb = torch.empty((nrow_g, nout, nchan_g, npol), dtype=torch.complex128, device=vis.device)
    xwt = torch.empty((nrow_g, nout, nchan_g, npol), dtype=torch.float64, device=vis.device)
    mfl = _model_flags(model_flags, fl)
    _lib.call("sdp_hip_point_sums", nt, nbl, nchan, npol, _ptr(vis), _ptr(model),
              _DT_CODE[vis.dtype], _ptr(weight), _ptr(fl), _ptr(mfl), fb, nrow_g, _ptr(row_ptr),
              _ptr(time_idx), int(nchan_g), int(nout), _ptr(perm), _ptr(conj), _ptr(xb),
              _ptr(xwt), _stream(vis.device))
    return xb, xwt


def _model_flags(model_flags, fl):
    """The model's own flags in the vis flags' dtype, or None."""
    if model_flags is None or fl is None:
        return None
    _on_gpu(model_flags, "model_flags")
    if model_flags.shape != fl.shape:
        raise ValueError("model flags must be shaped like vis")
    return model_flags.to(fl.dtype).contiguous()


def divide_vis(vis, model, weight, flags, model_flags=None):
    """(x, xwt) of divide_visibility, same shapes as vis."""
    _vis4(vis, "vis")
    _vis4(model, "model")
    if model.shape != vis.shape or model.dtype != vis.dtype:
        raise ValueError("model must match vis")
    fl, fb = _flags_of(flags, vis.shape)
    x = torch.empty_like(vis)
    xwt = torch.empty(vis.shape, dtype=torch.float64, device=vis.device)
    mfl = _model_flags(model_flags, fl)
    _lib.call("sdp_hip_divide_vis", vis.numel(), _ptr(vis), _ptr(model), _DT_CODE[vis.dtype],
              _ptr(weight), _ptr(fl), _ptr(mfl), fb, _ptr(x), _ptr(xwt), _stream(vis.device))
    return x, xwt


def apply_gains(vis, weight, flags, use_flags, ant1, ant2, time_row, gain, inverse):
    """apply_gaintable in place on device vis / weight [t, b, f, p]."""
    _vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if weight.shape != vis.shape or weight.dtype != torch.float64 or not weight.is_contiguous():
        raise ValueError("weight must be contiguous float64 shaped like vis")
    fl, fb = _flags_of(flags, vis.shape)
    _on_gpu(gain, "gain")
    if gain.dtype != torch.complex128 or gain.dim() != 5 or not gain.is_contiguous():
        raise ValueError("gain must be contiguous complex128 [rows, nants, nchan, nrec, nrec]")
    nrow_g, nants, nchan_g, nrec, _ = gain.shape
    _lib.call("sdp_hip_apply_gains", nt, nbl, nchan, npol, _ptr(vis), _DT_CODE[vis.dtype],
              _ptr(weight), _ptr(fl), fb, int(bool(use_flags)), _ptr(ant1), _ptr(ant2),
              _ptr(time_row), _ptr(gain), nrow_g, nants, nchan_g, nrec, int(bool(inverse)),
              _stream(vis.device))
    return vis, weight


GAIN_CHAIN_MAX = _lib.SDP_HIP_GAIN_CHAIN_MAX


def apply_gain_chain(vis, weight, ant1, ant2, time_rows, gains, inverse):
    """The gain tables ``gains`` (each complex128 [rows, nants, nchan_g, nrec,
    nrec]) with their time-row maps ``time_rows`` (each int32 [ntimes], -1 =
    no row) applied in order, in place on device vis / weight [t, b, f, p]:
    bit for bit what one ``apply_gains(..., use_flags=False)`` per table
    gives, in one pass over vis and weight per group of up to
    ``GAIN_CHAIN_MAX`` tables (sdp_hip_apply_gain_chain)."""
    _vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if weight.shape != vis.shape or weight.dtype != torch.float64 or not weight.is_contiguous():
        raise ValueError("weight must be contiguous float64 shaped like vis")
    gains, time_rows = list(gains), list(time_rows)
    if len(gains) != len(time_rows):
        raise ValueError("one time_row map per gain table")
    for a in (ant1, ant2):
        _on_gpu(a, "ant1 / ant2")
        if a.dtype != torch.int32 or a.numel() != nbl or not a.is_contiguous():
            raise ValueError("ant1 / ant2 must be contiguous int32 [nbl]")
    nants = gains[0].shape[1] if gains and gains[0].dim() == 5 else 1
    for g, tr in zip(gains, time_rows):
        _on_gpu(g, "gain")
        _on_gpu(tr, "time_row")
        if g.dtype != torch.complex128 or g.dim() != 5 or not g.is_contiguous():
            raise ValueError("gain must be contiguous complex128 [rows, nants, nchan, nrec, nrec]")
        if g.shape[1] != nants or g.shape[3] != g.shape[4]:
            raise ValueError("the tables of a chain share nants; gains are nrec x nrec")
        if tr.dtype != torch.int32 or tr.numel() != nt or not tr.is_contiguous():
            raise ValueError("time_row must be contiguous int32 [ntimes]")
    i32 = ctypes.c_int32
    for k0 in range(0, max(len(gains), 1), GAIN_CHAIN_MAX):  # an empty chain: the entry refuses
        gs, trs = gains[k0:k0 + GAIN_CHAIN_MAX], time_rows[k0:k0 + GAIN_CHAIN_MAX]
        n = len(gs)
        _lib.call("sdp_hip_apply_gain_chain", nt, nbl, nchan, npol, _ptr(vis),
                  _DT_CODE[vis.dtype], _ptr(weight), _ptr(ant1), _ptr(ant2), int(nants), n,
                  (ctypes.c_void_p * (n + 1))(*[g.data_ptr() for g in gs]),
                  (ctypes.c_void_p * (n + 1))(*[t.data_ptr() for t in trs]),
                  (i32 * (n + 1))(*[g.shape[0] for g in gs]),
                  (i32 * (n + 1))(*[g.shape[2] for g in gs]),
                  (i32 * (n + 1))(*[g.shape[3] for g in gs]), int(bool(inverse)),
                  _stream(vis.device))
    return vis, weight


# ---- visibility operations (sdp_hip_vis_average_channels / to_stokes / remove_continuum)
MAX_CONTINUUM_DEGREE = 5


def _f64_like(t, name, vis):
    _on_gpu(t, name)
    if t.shape != vis.shape or t.dtype != torch.float64 or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous float64 shaped like vis")
    return t


def _flags_required(flags, vis):
    if flags is None:
        raise ValueError("flags are required")
    return _flags_of(flags, vis.shape)


def vis_average_channels(vis, weight, imaging_weight, flags, group, variant):
    """Weighted channel averages over groups of ``group`` channels (which must
    divide nchan) of device arrays [t, b, f, p]: (vis, weight, imaging_weight,
    flags) shaped [t, b, f / group, p].  variant 0 is
    integrate_visibility_by_channel's arithmetic, 1
    average_visibility_by_channel's (include/ska_sdp_hip.h)."""
    _vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if group is None or int(group) != group or group < 1 or nchan % int(group):
        raise ValueError(f"the number of channels to average ({group}) must divide nchan = {nchan}")
    group = int(group)
    _f64_like(weight, "weight", vis)
    _f64_like(imaging_weight, "imaging_weight", vis)
    fl, fb = _flags_required(flags, vis)
    shape = (nt, nbl, nchan // group, npol)
    dev = vis.device
    ov = torch.empty(shape, dtype=vis.dtype, device=dev)
    ow = torch.empty(shape, dtype=torch.float64, device=dev)
    oiw = torch.empty(shape, dtype=torch.float64, device=dev)
    ofl = torch.empty(shape, dtype=fl.dtype, device=dev)
    _lib.call("sdp_hip_vis_average_channels", nt * nbl, nchan, npol, group, int(variant),
              _ptr(vis), _DT_CODE[vis.dtype], _ptr(weight), _ptr(imaging_weight), _ptr(fl), fb,
              _ptr(ov), _ptr(ow), _ptr(oiw), _ptr(ofl), fb, _stream(dev))
    return ov, ow, oiw, ofl


def vis_to_stokes(vis, flags, matrix):
    """convert_visibility_to_stokes in place on device vis / flags [t, b, f, 4]:
    vis <- matrix @ vis per sample (matrix: 4 x 4 complex, host), every pol's
    flag <- flag[0] | flag[3]."""
    import numpy as np
    _vis4(vis, "vis")
    if vis.shape[3] != 4:
        raise ValueError("stokesIQUV needs 4 polarisations")
    fl, fb = _flags_required(flags, vis)
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.complex128))
    if m.shape != (4, 4):
        raise ValueError("the conversion matrix must be 4 x 4")
    _lib.call("sdp_hip_vis_to_stokes", vis.numel() // 4, 4, _lib.SDP_HIP_STOKES_IQUV, _ptr(vis),
              _DT_CODE[vis.dtype], None, None, _ptr(fl), fb, ctypes.c_void_p(m.ctypes.data),
              None, None, None, None, fb, _stream(vis.device))
    return vis, fl


def vis_to_stokes_i(vis, weight, imaging_weight, flags):
    """convert_visibility_to_stokesI of device arrays [t, b, f, p] (p 2 or 4):
    new (vis, weight, imaging_weight, flags) shaped [t, b, f, 1]."""
    _vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if npol not in (2, 4):
        raise ValueError("stokesI needs 2 or 4 polarisations")
    _f64_like(weight, "weight", vis)
    _f64_like(imaging_weight, "imaging_weight", vis)
    fl, fb = _flags_required(flags, vis)
    shape = (nt, nbl, nchan, 1)
    dev = vis.device
    ov = torch.empty(shape, dtype=vis.dtype, device=dev)
    ow = torch.empty(shape, dtype=torch.float64, device=dev)
    oiw = torch.empty(shape, dtype=torch.float64, device=dev)
    ofl = torch.empty(shape, dtype=fl.dtype, device=dev)
    _lib.call("sdp_hip_vis_to_stokes", nt * nbl * nchan, npol, _lib.SDP_HIP_STOKES_I, _ptr(vis),
              _DT_CODE[vis.dtype], _ptr(weight), _ptr(imaging_weight), _ptr(fl), fb, None,
              _ptr(ov), _ptr(ow), _ptr(oiw), _ptr(ofl), fb, _stream(dev))
    return ov, ow, oiw, ofl


def vis_remove_continuum(vis, weight, flags, x, degree, mask=None, rank_capacity=None):
    """Fit and subtract a polynomial of ``degree`` in ``x`` [nchan] per
    (time, baseline, pol) spectrum, in place on device vis [t, b, f, p]
    (include/ska_sdp_hip.h).  Returns (deficient, count): the sorted indices
    row * npol + pol of the spectra with 1 <= n_live <= degree, which were
    left untouched, and their number; ``deficient`` is None when more than
    ``rank_capacity`` (default 2^20) were found."""
    _vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    if not 0 <= int(degree) <= MAX_CONTINUUM_DEGREE:
        raise ValueError(f"degree {degree}: the device fit takes degrees 0 to "
                         f"{MAX_CONTINUUM_DEGREE}")
    if nchan < 2:
        raise ValueError("remove_continuum needs at least 2 channels")
    _f64_like(weight, "weight", vis)
    fl, fb = _flags_of(flags, vis.shape)
    dev = vis.device
    _on_gpu(x, "x")
    if x.dtype != torch.float64 or tuple(x.shape) != (nchan,) or not x.is_contiguous():
        raise ValueError("x must be contiguous float64 [nchan]")
    if mask is not None:
        _on_gpu(mask, "mask")
        if tuple(mask.shape) != (nchan,):
            raise ValueError("mask must be [nchan]")
        mask = mask.to(torch.uint8).contiguous()
    nspec = nt * nbl * npol
    cap = 1 << 20 if rank_capacity is None else int(rank_capacity)
    cap = max(0, min(cap, nspec, 2 ** 31 - 1))
    rank_list = torch.empty((max(cap, 1),), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.call("sdp_hip_vis_remove_continuum", nt * nbl, nchan, npol, _ptr(vis),
              _DT_CODE[vis.dtype], _ptr(weight), _ptr(fl), fb, _ptr(x), _ptr(mask), int(degree),
              _ptr(rank_list), cap, _ptr(count), _stream(dev))
    n = int(count.item())
    if n > cap:
        return None, n
    return torch.sort(rank_list[:n]).values, n


# ---- CLEAN minor cycles (sdp_hip_clean_plane) --------------------------------
CLEAN_STOP = {0: "niter", 1: "threshold", 2: "zero"}


def _f64_plane(t, name, shape):
    _on_gpu(t, name)
    if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a contiguous float64 device tensor of shape {tuple(shape)}")
    return t


def clean_plane(algorithm, res, psf, comps, gain, pmax, absthresh, niter, window=None,
                sensitivity=None, coupling_diag=None, scale_kernels=None, scale_extent=0):
    """Up to ``niter`` CLEAN minor cycles of one plane, in place on device f64:
    ``res`` [S, ny, nx] (the residual; msclean: the scale-convolved stack),
    ``psf`` [S, S, py, px] (msclean: the scale cross terms), ``comps``
    [ny, nx]; optional ``window`` [S, ny, nx]; msclean also takes
    ``sensitivity`` [ny, nx], ``coupling_diag`` (S host floats) and
    ``scale_kernels`` [S, py, px], which ``scale_extent`` > 0 declares zero
    further than that many pixels from (py // 2, px // 2).  ``algorithm``
    "hogbom" (S = 1) or "msclean".  Returns (cycles run, "niter" | "threshold" | "zero")."""
    if algorithm not in ("hogbom", "msclean"):
        raise ValueError(f"unknown clean algorithm {algorithm}")
    ms = algorithm == "msclean"
    _on_gpu(res, "res")
    if res.dim() != 3 or psf.dim() != 4:
        raise ValueError("res must be [S, ny, nx] and psf [S, S, py, px]")
    ns, ny, nx = res.shape
    pny, pnx = psf.shape[2:]
    _f64_plane(res, "res", (ns, ny, nx))
    _f64_plane(psf, "psf", (ns, ns, pny, pnx))
    _f64_plane(comps, "comps", (ny, nx))
    if window is not None:
        _f64_plane(window, "window", (ns, ny, nx))
    if sensitivity is not None:
        _f64_plane(sensitivity, "sensitivity", (ny, nx))
    cd = None
    if ms:
        _f64_plane(scale_kernels, "scale_kernels", (ns, pny, pnx))
        cd = (ctypes.c_double * ns)(*[float(c) for c in coupling_diag])
    done, reason = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("sdp_hip_clean_plane",
              _lib.SDP_HIP_CLEAN_MSCLEAN if ms else _lib.SDP_HIP_CLEAN_HOGBOM, ns, ny, nx, pny,
              pnx, _ptr(res), _ptr(psf), _ptr(window), _ptr(sensitivity), cd,
              _ptr(scale_kernels if ms else None), int(scale_extent), _ptr(comps), float(gain), float(pmax), float(absthresh), int(niter),
              ctypes.byref(done), ctypes.byref(reason), _stream(res.device))
    return done.value, CLEAN_STOP[reason.value]


def clean_plane_complex(res, psf, comps, gain, pmax, absthresh, niter, window=None):
    """Up to ``niter`` complex Hogbom minor cycles of a Q / U pair cleaned as
    Q + iU, in place on device f64: ``res`` [2, ny, nx] (plane 0 Q, plane 1 U),
    ``psf`` [py, px] shared by both, ``comps`` [2, ny, nx]; optional ``window``
    [ny, nx].  The peak is the first maximum of hypot(q * w, u * w), the
    component (res[:, peak] * gain) * (1 / pmax), and the cycles stop once
    hypot(q, u) at the peak is below ``absthresh`` after the subtraction.
    Returns (cycles run, "niter" | "threshold")."""
    _on_gpu(res, "res")
    if res.dim() != 3 or res.shape[0] != 2 or psf.dim() != 2:
        raise ValueError("res must be [2, ny, nx] and psf [py, px]")
    _, ny, nx = res.shape
    pny, pnx = psf.shape
    _f64_plane(res, "res", (2, ny, nx))
    _f64_plane(psf, "psf", (pny, pnx))
    _f64_plane(comps, "comps", (2, ny, nx))
    if window is not None:
        _f64_plane(window, "window", (ny, nx))
    done, reason = ctypes.c_int(0), ctypes.c_int(0)
    _lib.call("sdp_hip_clean_plane_complex", ny, nx, pny, pnx, _ptr(res), _ptr(psf), _ptr(window),
              _ptr(comps), float(gain), float(pmax), float(absthresh), int(niter),
              ctypes.byref(done), ctypes.byref(reason), _stream(res.device))
    return done.value, CLEAN_STOP[reason.value]


# ---- msmfsclean minor cycles (sdp_hip_mfsclean_plane) ----------------------------
def mfsclean_plane(smresidual, m_model, ssmmpsf, scale_kernels, hsmmpsf, ihsmmpsf, gain, absthresh,
                   niter, findpeak="RASCIL", windowstack=None, sensitivity=None, scale_extent=0):
    """Up to ``niter`` multi-scale multi-frequency CLEAN minor cycles of one
    polarisation, in place on device f64: ``smresidual`` [S, T, ny, nx],
    ``m_model`` [T, ny, nx], ``ssmmpsf`` [S, S, 2T - 1, py, px] (plane k holds
    the moment pairs t + q = k), ``scale_kernels`` [S, py, px], which
    ``scale_extent`` > 0 declares zero further than that many pixels from
    (py // 2, px // 2); optional ``windowstack`` [S, ny, nx] and
    ``sensitivity`` [ny, nx]; ``hsmmpsf`` and ``ihsmmpsf`` [S, T, T] on the
    host.  ``findpeak`` "CASA" searches dchisq, anything else the principal
    solution's moment 0.  S <= 16, T <= 4.
    Returns (cycles run, "niter" | "threshold", cycles per scale)."""
    _on_gpu(smresidual, "smresidual")
    if smresidual.dim() != 4 or ssmmpsf.dim() != 5:
        raise ValueError("smresidual must be [S, T, ny, nx] and ssmmpsf [S, S, 2T - 1, py, px]")
    ns, nt, ny, nx = smresidual.shape
    pny, pnx = ssmmpsf.shape[3:]
    _f64_plane(smresidual, "smresidual", (ns, nt, ny, nx))
    _f64_plane(m_model, "m_model", (nt, ny, nx))
    _f64_plane(ssmmpsf, "ssmmpsf", (ns, ns, 2 * nt - 1, pny, pnx))
    _f64_plane(scale_kernels, "scale_kernels", (ns, pny, pnx))
    if windowstack is not None:
        _f64_plane(windowstack, "windowstack", (ns, ny, nx))
    if sensitivity is not None:
        _f64_plane(sensitivity, "sensitivity", (ny, nx))
    hess = []
    for name, h in (("hsmmpsf", hsmmpsf), ("ihsmmpsf", ihsmmpsf)):
        flat = [float(v) for scale in h for row in scale for v in row]
        if len(h) != ns or len(flat) != ns * nt * nt:
            raise ValueError(f"{name} must be a host array of shape {(ns, nt, nt)}")
        hess.append((ctypes.c_double * len(flat))(*flat))
    casa = findpeak == "CASA"
    done, reason = ctypes.c_int(0), ctypes.c_int(0)
    counts = (ctypes.c_int * ns)()
    _lib.call("sdp_hip_mfsclean_plane", ns, nt, ny, nx, pny, pnx, _ptr(smresidual), _ptr(m_model),
              _ptr(ssmmpsf), _ptr(scale_kernels), int(scale_extent), _ptr(windowstack),
              _ptr(sensitivity), ctypes.cast(hess[0], ctypes.c_void_p),
              ctypes.cast(hess[1], ctypes.c_void_p),
              _lib.SDP_HIP_MFSCLEAN_FINDPEAK_CASA if casa else _lib.SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL,
              float(gain), float(absthresh), int(niter), ctypes.byref(done), ctypes.byref(reason),
              ctypes.cast(counts, ctypes.c_void_p), _stream(smresidual.device))
    return done.value, CLEAN_STOP[reason.value], list(counts)


# ---- sky-component image operations (sdp_hip_skycomp_*) ----------------------
# (tile, component) pairs listed per launch; a longer list is split by component
# range into several launches, which keeps every pixel's order of addition
# (making the list takes about ten int64 temporaries per pair on the device)
SKYCOMP_MAX_PAIRS = 1 << 24
# restore leaves a component out of a tile where the exponent's argument
# exceeds this on the whole tile: exp(-700) ~ 1e-304
RESTORE_SKIP_ARGUMENT = 700.0


def _skycomp_image(image):
    _on_gpu(image, "image")
    if image.dim() != 4 or image.dtype not in (torch.float32, torch.float64) \
            or not image.is_contiguous():
        raise ValueError("image must be a contiguous float32 or float64 device tensor "
                         "[nchan, npol, ny, nx]")
    nchan, npol, ny, nx = image.shape
    if ny * nx >= 2 ** 31:
        raise ValueError("image planes of 2^31 pixels or more are not supported")
    return nchan * npol, ny, nx


def _tile_boxes(x_lo, x_hi, y_lo, y_hi, ny, nx):
    """Per component, the block of image tiles that its inclusive pixel box
    [x_lo, x_hi] x [y_lo, y_hi] meets: (first tile column, first tile row,
    tile columns, tiles in all); 0 tiles for a box off the image."""
    import numpy as np
    tx, ty = _lib.SDP_HIP_SKYCOMP_TILE_X, _lib.SDP_HIP_SKYCOMP_TILE_Y
    lim = lambda v, n: np.clip(np.asarray(v, dtype=np.float64), -1, n).astype(np.int64)
    x_lo, x_hi, y_lo, y_hi = lim(x_lo, nx), lim(x_hi, nx), lim(y_lo, ny), lim(y_hi, ny)
    on = (x_hi >= 0) & (x_lo <= nx - 1) & (y_hi >= 0) & (y_lo <= ny - 1) & (x_lo <= x_hi) \
        & (y_lo <= y_hi)
    tx0, tx1 = np.clip(x_lo, 0, nx - 1) // tx, np.clip(x_hi, 0, nx - 1) // tx
    ty0, ty1 = np.clip(y_lo, 0, ny - 1) // ty, np.clip(y_hi, 0, ny - 1) // ty
    ncols = np.where(on, tx1 - tx0 + 1, 0)
    return tx0, ty0, ncols, ncols * np.where(on, ty1 - ty0 + 1, 0)


def _tile_csr(boxes, start, stop, ny, nx, dev):
    """The per-tile component lists (CSR: tile_ptr int64 [ntiles + 1], tile_comp
    int32, ascending within a tile; tensors on ``dev``) of components start ..
    stop - 1, numbered from 0 at ``start``.  The (tile, component) pairs are
    written out component by component and sorted by tile, stably, on ``dev``;
    the host only knows how many there are."""
    tx0, ty0, ncols, cnt = (torch.as_tensor(b[start:stop], device=dev) for b in boxes)
    npairs = int(boxes[3][start:stop].sum())
    tiles_x = -(-nx // _lib.SDP_HIP_SKYCOMP_TILE_X)
    ntiles = tiles_x * -(-ny // _lib.SDP_HIP_SKYCOMP_TILE_Y)
    comp = torch.repeat_interleave(torch.arange(stop - start, device=dev), cnt, output_size=npairs)
    k = torch.arange(npairs, device=dev) - (torch.cumsum(cnt, 0) - cnt)[comp]
    w = ncols[comp]
    tile = (ty0[comp] + k // w) * tiles_x + tx0[comp] + k % w
    tile, order = torch.sort(tile, stable=True)
    ptr = torch.searchsorted(tile, torch.arange(ntiles + 1, device=dev))
    return ptr, comp[order].to(torch.int32)


def _skycomp_launches(boxes, ncomp):
    """Component ranges [start, stop) of at most SKYCOMP_MAX_PAIRS (tile,
    component) pairs each (a single component may exceed it)."""
    import numpy as np
    cum = np.cumsum(boxes[3])
    start = 0
    while start < ncomp:
        done = cum[start - 1] if start else 0
        stop = max(start + 1, int(np.searchsorted(cum, done + SKYCOMP_MAX_PAIRS, side="right")))
        yield start, min(stop, ncomp)
        start = min(stop, ncomp)


def _dev_array(a, dtype, dev):
    import numpy as np
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def skycomp_insert(image, origin, taps_y, taps_x, insertsum, flux):
    """insert_array for every component at once, in place on the device image
    [nchan, npol, ny, nx] (float64 or float32): component c adds
    flux[c, chan, pol] * ((taps_y[c, i] * taps_x[c, j]) / insertsum[c]) to
    pixel (origin[c, 1] + i, origin[c, 0] + j).  The component arrays are host
    arrays: origin [ncomp, 2] integers (x0, y0), taps [ncomp, L], insertsum
    [ncomp], flux [ncomp, nchan, npol].  Pixels add their terms in component
    order (include/ska_sdp_hip.h): the result is numpy's sequential one."""
    import numpy as np
    nplanes, ny, nx = _skycomp_image(image)
    origin = np.asarray(origin, dtype=np.int64).reshape(-1, 2)
    ncomp = origin.shape[0]
    if ncomp == 0:
        return image
    taps_y = np.asarray(taps_y, dtype=np.float64).reshape(ncomp, -1)
    taps_x = np.asarray(taps_x, dtype=np.float64).reshape(ncomp, -1)
    L = taps_y.shape[1]
    flux = np.asarray(flux, dtype=np.float64)
    insertsum = np.asarray(insertsum, dtype=np.float64)
    if L < 1 or taps_x.shape[1] != L or flux.shape != (ncomp,) + tuple(image.shape[:2]) \
            or insertsum.shape != (ncomp,):
        raise ValueError("skycomp_insert: component arrays do not match")
    if np.abs(origin).max() >= 2 ** 30:
        raise ValueError("skycomp_insert: window origin out of range")
    dev = image.device
    boxes = _tile_boxes(origin[:, 0], origin[:, 0] + L - 1, origin[:, 1], origin[:, 1] + L - 1,
                        ny, nx)
    for s, e in _skycomp_launches(boxes, ncomp):
        if not boxes[3][s:e].any():
            continue
        args = [_dev_array(a, dt, dev) for a, dt in (
            (origin[s:e], np.int32), (taps_y[s:e], np.float64), (taps_x[s:e], np.float64),
            (insertsum[s:e], np.float64), (flux[s:e], np.float64))]
        args += _tile_csr(boxes, s, e, ny, nx, dev)
        _lib.call("sdp_hip_skycomp_insert", nplanes, ny, nx, _ptr(image), _DT_CODE[image.dtype],
                  e - s, L, *[_ptr(a) for a in args], _stream(dev))
    return image


def skycomp_restore(image, xy, flux, a, b, c):
    """restore_skycomponent's sum, in place on the device image [nchan, npol,
    ny, nx]: component k at pixel xy[k] = (x, y) adds flux[k, chan, pol] *
    exp(-(a dx^2 + b dx dy + c dy^2)), dx = column - x, dy = row - y, the
    components added per pixel in their order.  xy [ncomp, 2] and flux [ncomp,
    nchan, npol] are host arrays.  A component is left out of an image tile
    only where the argument exceeds RESTORE_SKIP_ARGUMENT on all of it: the
    argument is at least lmin d^2, lmin the smaller eigenvalue of the
    quadratic form and d the distance to the component."""
    import numpy as np
    nplanes, ny, nx = _skycomp_image(image)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ncomp = xy.shape[0]
    if ncomp == 0:
        return image
    flux = np.asarray(flux, dtype=np.float64)
    if flux.shape != (ncomp,) + tuple(image.shape[:2]):
        raise ValueError("skycomp_restore: flux must be [ncomp, nchan, npol]")
    if not np.isfinite(xy).all():
        raise ValueError("skycomp_restore: a component has no pixel location")
    a, b, c = float(a), float(b), float(c)
    lmin = 0.5 * ((a + c) - np.hypot(a - c, b)) * (1.0 - 1e-9)
    # the box of radius r + 1 around a component holds every pixel within r
    r = np.sqrt(RESTORE_SKIP_ARGUMENT / lmin) + 1.0 if lmin > 0.0 else np.inf
    boxes = _tile_boxes(np.floor(xy[:, 0] - r), np.ceil(xy[:, 0] + r),
                        np.floor(xy[:, 1] - r), np.ceil(xy[:, 1] + r), ny, nx)
    dev = image.device
    for s, e in _skycomp_launches(boxes, ncomp):
        if not boxes[3][s:e].any():
            continue
        xy_d, flux_d = _dev_array(xy[s:e], np.float64, dev), _dev_array(flux[s:e], np.float64, dev)
        ptr, comp = _tile_csr(boxes, s, e, ny, nx, dev)
        _lib.call("sdp_hip_skycomp_restore", nplanes, ny, nx, _ptr(image), _DT_CODE[image.dtype],
                  e - s, _ptr(xy_d), _ptr(flux_d), a, b, c, _ptr(ptr), _ptr(comp), _stream(dev))
    return image


def skycomp_nearest(ny, nx, xy, dev):
    """The label image [ny, nx] (int64, on ``dev``) of the nearest of the points
    xy [ncomp, 2] = (x, y) (host): argmin_c hypot(row - y_c, column - x_c),
    the first minimum on ties."""
    import numpy as np
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    if xy.shape[0] < 1:
        raise ValueError("skycomp_nearest needs at least one point")
    if ny * nx >= 2 ** 31:
        raise ValueError("image planes of 2^31 pixels or more are not supported")
    pts = _dev_array(xy, np.float64, dev)
    _on_gpu(pts, "points")
    labels = torch.empty((ny, nx), dtype=torch.int64, device=dev)
    _lib.call("sdp_hip_skycomp_nearest", int(ny), int(nx), xy.shape[0], _ptr(pts), _ptr(labels),
              _stream(dev))
    return labels


# ---- plane mixing: frequency Taylor terms (sdp_hip_mix_planes) ----------------
# planes the kernel holds in registers per pixel: with min(nin, nout) at most
# this, every plane is read once and written once
MIX_PLANES_REGS = _lib.SDP_HIP_MIX_PLANES_REGS
MIX_PLANES_MAX = _lib.SDP_HIP_MIX_PLANES_MAX
MIX_NAN_INPUT = _lib.SDP_HIP_MIX_NAN_INPUT
MIX_NAN_OUTPUT = _lib.SDP_HIP_MIX_NAN_OUTPUT


def _plane_list(x, name):
    """The planes of a cube (its first axis) or of a list of tensors."""
    if isinstance(x, torch.Tensor):
        if x.dim() < 2:
            raise ValueError(f"{name}: a cube needs a plane axis in front of the pixel axes")
        return [x[i] for i in range(x.shape[0])]
    return list(x)


def _byte_ranges(planes):
    import numpy as np
    start = np.array([p.data_ptr() for p in planes], dtype=np.uint64)
    return start, start + np.array([p.numel() * p.element_size() for p in planes], dtype=np.uint64)


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
    ins = _plane_list(inputs, "inputs")
    if not ins:
        raise ValueError("mix_planes needs at least one input plane")
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != len(ins) or w.shape[0] < 1:
        raise ValueError(f"weights must be [nout, nin = {len(ins)}], not {w.shape}")
    nout, nin = w.shape
    if max(nin, nout) > MIX_PLANES_MAX:
        raise ValueError(f"mix_planes takes at most {MIX_PLANES_MAX} input and as many output "
                         f"planes, not {nin} and {nout}")
    first = _on_gpu(ins[0], "inputs")
    dev, npix = first.device, first.numel()
    if first.dtype not in (torch.float32, torch.float64) or npix < 1:
        raise ValueError("the input planes must be non-empty float32 or float64 tensors")
    for p in ins:
        _on_gpu(p, "inputs")
        if p.dtype != first.dtype or p.device != dev or p.numel() != npix:
            raise ValueError("the input planes must agree in dtype, device and size")
        if not p.is_contiguous():
            raise ValueError("every input plane must be contiguous")
    result = outputs
    if outputs is None:
        result = outputs = _alloc((nout,) + tuple(first.shape), torch.float64, dev)
    outs = _plane_list(outputs, "outputs")
    if len(outs) != nout:
        raise ValueError(f"{len(outs)} output planes for {nout} rows of weights")
    for p in outs:
        _on_gpu(p, "outputs")
        if p.dtype != torch.float64 or p.device != dev or p.numel() != npix:
            raise ValueError("the output planes must be float64 on the inputs' device and of "
                             "their size")
        if not p.is_contiguous():
            raise ValueError("every output plane must be contiguous")
    i_lo, i_hi = _byte_ranges(ins)
    o_lo, o_hi = _byte_ranges(outs)
    if ((o_lo[:, None] < i_hi[None, :]) & (i_lo[None, :] < o_hi[:, None])).any():
        raise ValueError("an output plane overlaps an input plane")
    order = np.argsort(o_lo)
    if (o_hi[order][:-1] > o_lo[order][1:]).any():
        raise ValueError("two output planes overlap")
    in_tab = (ctypes.c_void_p * nin)(*[p.data_ptr() for p in ins])
    out_tab = (ctypes.c_void_p * nout)(*[p.data_ptr() for p in outs])
    if stream is None:
        st = _stream(dev)
    else:
        st = ctypes.c_void_p(getattr(stream, "cuda_stream", stream))
    seen = ctypes.c_int(0)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_mix_planes", nin, nout, npix, ctypes.cast(in_tab, ctypes.c_void_p),
                  _DT_CODE[first.dtype], ctypes.cast(out_tab, ctypes.c_void_p),
                  ctypes.c_void_p(w.ctypes.data),
                  ctypes.byref(seen) if check_nan else ctypes.POINTER(ctypes.c_int)(), st)
    return (result, seen.value) if check_nan else result


# ---- gather of image facets (sdp_hip_gather_facets) -----------------------------
GATHER_FACETS_MAX = _lib.SDP_HIP_GATHER_FACETS_MAX


def _gather_facets_call(tabs, facets, lead, facet_shape, image_shape, origin, step, taper_y,
                        taper_x, normalise, want_image, want_weights, dtype, dev, stream):
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
    out = _alloc(shape, dtype, dev) if want_image else None
    sumwt = _alloc(shape, dtype, dev) if want_weights else None
    if stream is None:
        st = _stream(dev)
    else:
        st = ctypes.c_void_p(getattr(stream, "cuda_stream", stream))
    null = ctypes.c_void_p(0)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_gather_facets", _DT_CODE[dtype], int(facets), nplanes, int(ny), int(nx),
                  int(dy), int(dx), int(y0), int(x0), int(sy), int(sx),
                  *([null] * 3 if tabs is None else [ctypes.c_void_p(t.ctypes.data) for t in tabs]),
                  *[null if t is None else ctypes.c_void_p(t.ctypes.data) for t in tapers],
                  int(bool(normalise)), _ptr(out), _ptr(sumwt), st)
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
    first = _on_gpu(facet_list[0], "facet_list")
    if first.dim() < 3:
        raise ValueError("a facet needs a plane axis in front of its two pixel axes")
    lead, nlead = tuple(first.shape[:-2]), first.dim() - 2
    tabs = [np.empty(len(facet_list), dtype=np.uint64), np.empty(len(facet_list), dtype=np.int64),
            np.empty(len(facet_list), dtype=np.int64)]
    for f, t in enumerate(facet_list):
        _on_gpu(t, "facet_list")
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
        tabs[0][f], tabs[1][f], tabs[2][f] = t.data_ptr(), pstride, t.stride(-2)
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


# ---- image segmentation: find_skycomponents (sdp_hip_segment_*) -------------------
SEGMENT_KERNEL_MAX = _lib.SDP_HIP_SEGMENT_KERNEL_MAX


def _segment_planes(planes, name):
    """The planes [nplanes, ny, nx] of a segmentation call: a float32 or float64
    device tensor whose planes are contiguous and evenly spaced, such as a cube
    or ``pixels[:, 0]`` of an image."""
    _on_gpu(planes, name)
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
    labels = _alloc((ny, nx), torch.int32, dev)
    count = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    keep = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)  # non-finite flag, nlabels
    with torch.cuda.device(dev):
        st = _stream(dev)
        _lib.call("sdp_hip_segment_label", nchan, ny, nx, _ptr(planes), _DT_CODE[planes.dtype],
                  stride, taps.shape[0], ctypes.c_void_p(taps.ctypes.data), tap_sum, threshold,
                  _ptr(labels), _ptr(count), _ptr(state), st)
        _lib.call("sdp_hip_segment_roots", ny, nx, _ptr(labels), _ptr(count),
                  int(min(max(int(npixels), 0), 2 ** 31 - 1)), _ptr(keep), st)
        rank = torch.cumsum(keep.view(-1), 0, dtype=torch.int32)
        _lib.call("sdp_hip_segment_relabel", ny, nx, _ptr(labels), _ptr(keep), _ptr(rank),
                  _ptr(labels), st)
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
    _on_gpu(labels, "labels")
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
            _lib.call("sdp_hip_segment_peaks", nplanes, ny, nx, _ptr(planes),
                      _DT_CODE[planes.dtype], stride, _ptr(labels), nlabels, _ptr(values),
                      _ptr(indices), _stream(dev))
    return values, indices


# ---- batched 2-D Gaussian fits: fit_skycomponent (sdp_hip_gauss_fit) ---------------
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
    first = _on_gpu(planes[0], "planes")
    if first.dtype not in (torch.float32, torch.float64):
        raise ValueError("gauss_fit: the planes must be float32 or float64")
    ptrs = np.empty(nfit, dtype=np.uint64)
    strides = np.empty(nfit, dtype=np.int64)
    seen = {}
    for f, t in enumerate(planes):
        key = id(t)
        if key not in seen:
            _on_gpu(t, "planes")
            if t.dim() != 2 or t.dtype != first.dtype or t.device != first.device:
                raise ValueError("gauss_fit: the planes must be 2-D and agree in dtype and device")
            if t.shape[1] > 1 and t.stride(1) != 1:
                raise ValueError("gauss_fit: the x stride of every plane must be 1")
            if t.stride(0) < 0:
                raise ValueError("gauss_fit: a row stride is negative")
            seen[key] = (t.data_ptr(), t.stride(0), int(t.shape[0]), int(t.shape[1]))
        ptrs[f], strides[f], ny, nx = seen[key]
        if not (0 <= x0[f] and x0[f] + GAUSS_FIT_WINDOW <= nx
                and 0 <= y0[f] and y0[f] + GAUSS_FIT_WINDOW <= ny):
            raise ValueError(f"gauss_fit: the window of fit {f} at row {y0[f]}, column {x0[f]} "
                             f"does not lie on its plane of {ny} x {nx} pixels")
    x0 = np.ascontiguousarray(x0, dtype=np.int32)
    y0 = np.ascontiguousarray(y0, dtype=np.int32)
    dev = first.device
    params = _alloc((nfit, 6), torch.float64, dev)
    status = torch.empty(nfit, dtype=torch.int32, device=dev)
    niter = torch.empty(nfit, dtype=torch.int32, device=dev)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_gauss_fit", nfit, host(ptrs), _DT_CODE[first.dtype], host(strides),
                  host(x0), host(y0), max_iter, _ptr(params), _ptr(status), _ptr(niter),
                  _stream(dev))
    return params, status, niter


# ---- bandpass resampling (sdp_hip_resample_polyfit / _interp) ------------------
BANDPASS_MAX_DEGREE = _lib.SDP_HIP_BANDPASS_MAX_DEGREE
BANDPASS_MAX_SEGMENTS = _lib.SDP_HIP_BANDPASS_MAX_SEGMENTS


def _bandpass_gain(gain):
    """(rows, c_in, nrec) of a gain table [T, A, C_in, R, R] complex128 on the device."""
    _on_gpu(gain, "gain")
    if gain.dim() != 5 or gain.dtype != torch.complex128 or gain.shape[3] != gain.shape[4] \
            or gain.shape[3] not in (1, 2):
        raise ValueError("gain must be a complex128 device tensor [time, ant, chan, rec, rec] "
                         "with rec 1 or 2")
    if not gain.is_contiguous():
        raise ValueError("gain must be contiguous")
    if gain.shape[0] * gain.shape[1] < 1:
        raise ValueError("gain holds no spectra")
    return int(gain.shape[0] * gain.shape[1]), int(gain.shape[2]), int(gain.shape[3])


def resample_polyfit(gain, q, e, seg, edges):
    """Least-squares polynomial resampling of every spectrum of ``gain``
    [T, A, C_in, R, R] (complex128, contiguous, on the device) onto C_out
    channels: a new device tensor [T, A, C_out, R, R] (include/ska_sdp_hip.h).

    The fit is handed over as host tables (numpy), built by
    ``calibration.beamformer_utils.polyfit_tables``: ``q`` [degree + 1, C_in]
    and ``e`` [C_out, degree + 1] float64, the values of the polynomials
    orthonormal on each segment's input channels, ``seg`` [C_out] the segment
    of every output channel (-1: none, written NaN + NaN j) and ``edges``
    [nseg + 1] the segments' first channels, ending with C_in."""
    import numpy as np
    nrows, c_in, nrec = _bandpass_gain(gain)
    q = np.ascontiguousarray(q, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    if q.ndim != 2 or e.ndim != 2 or seg.ndim != 1 or edges.ndim != 1:
        raise ValueError("q and e must be 2-D, seg and edges 1-D")
    nd, c_out, nseg = q.shape[0], e.shape[0], len(edges) - 1
    if not 1 <= nd <= BANDPASS_MAX_DEGREE + 1:
        raise ValueError(f"degree {nd - 1}: the device fit takes degrees 0 to {BANDPASS_MAX_DEGREE}")
    if not 1 <= nseg <= BANDPASS_MAX_SEGMENTS:
        raise ValueError(f"{nseg} segments: the device fit takes 1 to {BANDPASS_MAX_SEGMENTS}")
    if c_in < 2:
        raise ValueError("resampling needs at least 2 input channels")
    if q.shape != (nd, c_in) or e.shape != (c_out, nd) or seg.shape != (c_out,) or c_out < 1:
        raise ValueError(f"tables do not fit: q {q.shape}, e {e.shape}, seg {seg.shape} for "
                         f"{c_in} input channels")
    if edges[0] < 0 or edges[-1] > c_in or np.any(np.diff(edges) < 0):
        raise ValueError(f"edges {edges} must ascend within 0 .. {c_in}")
    if np.any(seg < -1) or np.any(seg >= nseg):
        raise ValueError(f"seg must lie in -1 .. {nseg - 1}")
    dev = gain.device
    out = _alloc(tuple(gain.shape[:2]) + (c_out, nrec, nrec), torch.complex128, dev)
    tabs = [torch.as_tensor(a, device=dev) for a in (q, e, seg, edges)]
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_resample_polyfit", nrows, c_in, c_out, nrec, nd - 1, nseg, _ptr(gain),
                  _ptr(out), *[_ptr(t) for t in tabs], _stream(dev))
    return out


def resample_interp(gain, x_in, x_out, interval):
    """numpy.interp of every spectrum of ``gain`` [T, A, C_in, R, R]
    (complex128, contiguous, on the device) from the abscissae ``x_in``
    [C_in] to ``x_out`` [C_out], bit for bit: a new device tensor
    [T, A, C_out, R, R].  ``interval`` [C_out] (host, from
    ``calibration.beamformer_utils.interp_intervals``) is the knot interval
    of every output point as include/ska_sdp_hip.h encodes it."""
    import numpy as np
    nrows, c_in, nrec = _bandpass_gain(gain)
    x_in = np.ascontiguousarray(x_in, dtype=np.float64)
    x_out = np.ascontiguousarray(x_out, dtype=np.float64)
    interval = np.ascontiguousarray(interval, dtype=np.int32)
    c_out = len(x_out)
    if x_in.shape != (c_in,) or x_out.ndim != 1 or interval.shape != (c_out,) or c_out < 1:
        raise ValueError(f"tables do not fit: x_in {x_in.shape}, x_out {x_out.shape}, interval "
                         f"{interval.shape} for {c_in} input channels")
    if np.any(interval < -2):
        raise ValueError("interval must be -2, -1 or a knot index")
    dev = gain.device
    out = _alloc(tuple(gain.shape[:2]) + (c_out, nrec, nrec), torch.complex128, dev)
    tabs = [torch.as_tensor(a, device=dev) for a in (x_in, x_out, interval)]
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_resample_interp", nrows, c_in, c_out, nrec, _ptr(gain), _ptr(out),
                  *[_ptr(t) for t in tabs], _stream(dev))
    return out


# ---- sums of imaging results and clean thresholds (sdp_hip_sum_planes, sdp_hip_peak_abs) ----
SUM_PLANES_MAX = _lib.SDP_HIP_SUM_PLANES_MAX
PEAK_NAN_INPUT = _lib.SDP_HIP_PEAK_NAN_INPUT
PEAK_NAN_MEAN = _lib.SDP_HIP_PEAK_NAN_MEAN
_PEAK_MODES = {"moment0": _lib.SDP_HIP_PEAK_MOMENT0, "refchan": _lib.SDP_HIP_PEAK_REFCHAN}


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
    first = _on_gpu(ins[0], "inputs")
    dev, shape, dtype = first.device, tuple(first.shape), first.dtype
    real = (torch.float32, torch.float64)
    if dtype not in (real if weights is not None else real + (torch.complex64, torch.complex128)) \
            or first.numel() < 1:
        raise ValueError("the inputs must be non-empty float32 or float64 tensors (or, without "
                         "weights, complex64 or complex128)")
    for t in ins:
        _on_gpu(t, "inputs")
        if t.dtype != dtype or t.device != dev or tuple(t.shape) != shape:
            raise ValueError("the inputs must agree in dtype, device and shape")
    if out is None:
        out = _alloc(shape, dtype, dev)
    _on_gpu(out, "out")
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
        w_dev = _dev_array(w.reshape(len(ins), nplane), np.float64, dev)
        norm, s_dev = int(bool(normalise)), None
        if norm:
            if sumwt is None:
                raise ValueError("normalising needs sumwt")
            s = np.array(sumwt, dtype=np.float64)
            if s.shape != lead:
                raise ValueError(f"sumwt must be {lead}, not {s.shape}")
            s_dev = _dev_array(s.reshape(nplane), np.float64, dev)
    o_lo, o_hi = _byte_ranges([res])
    i_lo, i_hi = _byte_ranges(cubes)
    clash = (o_lo < i_hi) & (i_lo < o_hi)
    if weights is None and cubes[0].data_ptr() == res.data_ptr():
        clash[0] = False  # the sum onto its first entry
    if clash.any():
        raise ValueError("out overlaps an input")
    tab = (ctypes.c_void_p * len(cubes))(*[t.data_ptr() for t in cubes])
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_sum_planes", len(cubes), nplane, nelem // nplane,
                  ctypes.cast(tab, ctypes.c_void_p), _DT_CODE[res.dtype], _ptr(res), _ptr(w_dev),
                  _ptr(s_dev), norm, _stream(dev))
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
    _on_gpu(cube, "cube")
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
        _lib.call("sdp_hip_peak_abs", _PEAK_MODES[mode], nchan, npol, ny, nx, _ptr(cube),
                  _DT_CODE[cube.dtype], cs, ps, rs, ctypes.byref(peak), ctypes.byref(seen),
                  _stream(cube.device))
    value = peak.value
    if mode == "refchan" and seen.value & PEAK_NAN_INPUT:
        value = float("nan")
    return value, seen.value
