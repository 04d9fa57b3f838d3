"""The w-stacking gridder (csrc/wstack.hip): ms2dirty / dirty2ms and their
fused, batched and per-pol forms, the layout queries and the workspace."""

import ctypes
import logging

import torch

from .. import _lib
from ._operands import DT_CODE, FLAG_BYTES, alloc, check_uvw, host_doubles, on_gpu, ptr, stream

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
_COMPLEX = (torch.complex64, torch.complex128)


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


# ---- the checks and argument runs the seven gridder wrappers share ------------
def _prologue(uvw, freq, epsilon, precision):
    """The operands every wrapper starts from: (device, freq as contiguous
    f64, nrow, nchan, precision flag bits)."""
    pbits = _prec_bits(epsilon, precision)
    check_uvw(uvw)
    freq = on_gpu(freq, "freq").to(torch.float64).contiguous()
    return uvw.device, freq, uvw.shape[0], freq.shape[0], pbits


def _check_vis(vis, nrow, nchan, ndim, name="vis"):
    """``vis`` (or a visibility output) is complex [nrow, nchan] (ndim 2) or
    [nrow, nchan, npol] (ndim 3)."""
    on_gpu(vis, name)
    if vis.dtype not in _COMPLEX or vis.dim() != ndim or tuple(vis.shape[:2]) != (nrow, nchan):
        raise ValueError(f"{name} must be complex [nrow, nchan{', npol' if ndim == 3 else ''}]")


def _check_wgt(wgt, nrow, nchan, ndim=2):
    """ducc0 takes f64 weights; f32 (the bench's) and f64 are both read in
    place.  [nrow, nchan] weights may be None, [nrow, nchan, npol] not."""
    if wgt is None and ndim == 2:
        return
    on_gpu(wgt, "wgt")
    if wgt.dtype not in (torch.float32, torch.float64) or wgt.dim() != ndim \
            or tuple(wgt.shape[:2]) != (nrow, nchan):
        raise ValueError("wgt must be float32 or float64 "
                         f"[nrow, nchan{', npol' if ndim == 3 else ''}]")


def _coef_buffer(coef, nrows, npv):
    """The pol conversion as interleaved (re, im) host doubles, or None: a
    vector of ``npv`` complex entries (``nrows`` None) or a matrix
    [nrows][npv], row-major."""
    if coef is None:
        return None
    if nrows is None:
        rows = [[complex(x) for x in coef]]
        if len(rows[0]) != npv:
            raise ValueError("coef must have one entry per visibility pol")
    else:
        rows = [[complex(z) for z in r] for r in coef]
        if len(rows) != nrows or any(len(r) != npv for r in rows):
            raise ValueError("coef must be [npol_img][npol_vis]")
    return host_doubles(v for r in rows for z in r for v in (z.real, z.imag))


def _dirty_out(out, out_strides, shape, dev, may_release=True):
    """The f64 dirty output and its element strides: a new tensor of ``shape``
    when ``out`` is None, else ``out`` with the strides given or its own."""
    if out is None:
        out, out_strides = alloc(shape, torch.float64, dev, may_release), None
    if out_strides is None:
        out_strides = out.stride()
    on_gpu(out, "out")
    if out.dtype != torch.float64:
        raise ValueError("dirty output must be float64")
    return out, out_strides


def _dirty_in(dirty, dirty_strides, npix, ndim):
    """(npix_x, npix_y, strides) of the f64 image (ndim 2) or [npol_img, nx,
    ny] stack of images (ndim 3) a predict reads."""
    on_gpu(dirty, "dirty")
    if dirty.dtype != torch.float64 or (ndim == 3 and dirty.dim() != 3):
        raise ValueError("dirty must be float64" + (" [npol_img, nx, ny]" if ndim == 3 else ""))
    npix_x, npix_y = (dirty.shape[-2], dirty.shape[-1]) if npix is None else npix
    if dirty_strides is None:
        dirty_strides = dirty.stride()[-ndim:]
    return npix_x, npix_y, dirty_strides


def _check_bounds(bounds):
    if len(bounds) != 6:
        raise ValueError("bounds: {wmin, wmax, umax, vmax, fmin, fmax}")


def _flag_bits(flip_uw, accumulate, pbits, **named_bits):
    """The C ABI's flag word: ``name=truth`` sets SDP_HIP_<NAME>."""
    bits = ((_lib.SDP_HIP_FLIP_UW if flip_uw else 0) | (_lib.SDP_HIP_ACCUMULATE if accumulate else 0)
            | pbits)
    for name, on in named_bits.items():
        if on:
            bits |= getattr(_lib, "SDP_HIP_" + name.upper())
    return bits


def _uvw_args(uvw, freq, nchan, nrow):
    return ptr(uvw), uvw.stride(0), ptr(freq), nchan, nrow


def _strided_args(t, ndim, none_code, codes=DT_CODE):
    """(pointer, dtype code, element strides) of an operand of ``ndim`` axes
    read or written in place; NULL, ``none_code`` and zeros for None."""
    if t is None:
        return (ptr(None), none_code) + (0,) * ndim
    return (ptr(t), codes[t.dtype], *t.stride())


def _flag_args(flags):
    return _strided_args(flags, 3, 0, FLAG_BYTES)


def _grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits):
    return (int(npix_x), int(npix_y), float(pixsize_x), float(pixsize_y), float(epsilon),
            int(bool(do_wstacking)), bits)


# ---- the wrappers ----------------------------------------------------------------
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
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    if vis is not None:
        _check_vis(vis, nrow, nchan, 2)
    _check_wgt(wgt, nrow, nchan)
    out, out_strides = _dirty_out(out, out_strides, (npix_x, npix_y), dev)
    bits = _flag_bits(flip_uw, accumulate, pbits, slot1=slot)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty", *_uvw_args(uvw, freq, nchan, nrow),
        *_strided_args(vis, 2, _lib.SDP_HIP_C64), *_strided_args(wgt, 2, _lib.SDP_HIP_F32),
        *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
        ptr(out), int(out_strides[0]), int(out_strides[1]), stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def uvw_bounds(uvw, freq):
    """Host {min w, max w, max|u|, max|v|, min f, max f} of device arrays uvw
    [nrow, 3] (metres) and freq: one batch's contribution to the bounds of
    an ms2dirty_batch sequence (combine with merge_bounds)."""
    check_uvw(uvw)
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
    _check_bounds(bounds)
    bbuf = host_doubles(bounds)
    bits = _flag_bits(flip_uw, False, _prec_bits(epsilon, precision))
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_wstack_layout", bbuf,
              *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
              ctypes.byref(info))
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
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    if vis is not None:
        _check_vis(vis, nrow, nchan, 2)
    _check_wgt(wgt, nrow, nchan)
    if last:
        # (never auto-release the workspace past the first batch: it holds the
        # sequence's resident planes)
        out, out_strides = _dirty_out(out, out_strides, (npix_x, npix_y), dev, may_release=first)
    else:
        out, out_strides = None, (0, 0)
    _check_bounds(bounds)
    vals = [float(x) for x in bounds]
    if slab is not None:
        lo, hi = (int(x) for x in slab)
        if not 0 <= lo < hi:
            raise ValueError("slab: first planes (lo, hi) with 0 <= lo < hi")
        vals += [float(lo), float(hi)]
    bits = _flag_bits(flip_uw, accumulate, pbits, batch_first=first, batch_last=last,
                      w_slab=slab is not None)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty_batch", *_uvw_args(uvw, freq, nchan, nrow),
        *_strided_args(vis, 2, _lib.SDP_HIP_C64), *_strided_args(wgt, 2, _lib.SDP_HIP_F32),
        *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
        host_doubles(vals), ptr(out), int(out_strides[0]), int(out_strides[1]), stream(dev),
        ctypes.byref(info))
    return out, info.as_dict()


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
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    npv = 1
    if vis is not None:
        _check_vis(vis, nrow, nchan, 3)
        npv = vis.shape[2]
    if flags is not None:
        on_gpu(flags, "flags")
        if flags.dtype not in FLAG_BYTES or flags.dim() != 3 or tuple(flags.shape[:2]) != (nrow, nchan):
            raise ValueError("flags must be an integer [nrow, nchan, npol] tensor")
        npv = max(npv, flags.shape[2])
    _check_wgt(wgt, nrow, nchan)
    if not 0 <= pol < npv:
        raise ValueError("pol out of range")
    cbuf = _coef_buffer(coef, None, npv)
    out, out_strides = _dirty_out(out, out_strides, (npix_x, npix_y), dev)
    if sumwt is not None and (sumwt.dtype != torch.float64 or not sumwt.is_cuda):
        raise ValueError("sumwt must be a float64 device tensor")
    batched = bounds is not None
    if batched:
        _check_bounds(bounds)
    bits = _flag_bits(flip_uw, accumulate, pbits, keep_buckets=keep_buckets,
                      reuse_buckets=reuse_buckets, slot1=slot, batch_first=batched and first,
                      batch_last=batched and last)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty_vis_batch" if batched else "sdp_hip_ms2dirty_vis",
        *_uvw_args(uvw, freq, nchan, nrow), *_strided_args(vis, 3, _lib.SDP_HIP_C64), npv, cbuf,
        *_strided_args(wgt, 2, _lib.SDP_HIP_F32), *_flag_args(flags), int(pol),
        *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
        *((host_doubles(bounds),) if batched else ()),
        ptr(out), int(out_strides[0]), int(out_strides[1]), ptr(sumwt), host_doubles(shift_lmn, 3),
        stream(dev), ctypes.byref(info))
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
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    _check_vis(vis, nrow, nchan, 3)
    npv = vis.shape[2]
    if flags is not None:
        on_gpu(flags, "flags")
        if flags.dtype not in FLAG_BYTES or tuple(flags.shape) != tuple(vis.shape):
            raise ValueError("flags must be an integer tensor shaped as vis")
    _check_wgt(wgt, nrow, nchan, 3)
    npo = npv if coef is None else len(coef)
    if not 1 <= npo <= min(npv, wgt.shape[2]):
        raise ValueError("npol_img must be 1..npol_vis (and have weights)")
    cbuf = _coef_buffer(coef, npo, npv)
    out, out_strides = _dirty_out(out, out_strides, (npo, npix_x, npix_y), dev)
    if sumwt is not None and (sumwt.dtype != torch.float64 or not sumwt.is_cuda or
                              sumwt.numel() < npo):
        raise ValueError("sumwt must be a float64 device tensor with one entry per image pol")
    bits = _flag_bits(flip_uw, accumulate, pbits)
    info = _lib.WGridInfo()
    _lib.call(
        "sdp_hip_ms2dirty_vis_pols",
        *_uvw_args(uvw, freq, nchan, nrow), *_strided_args(vis, 3, None), npv, cbuf, npo,
        *_strided_args(wgt, 3, None), *_flag_args(flags),
        *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
        ptr(out), int(out_strides[1]), int(out_strides[2]), int(out_strides[0]),
        ptr(sumwt), int(sumwt.stride(0)) if sumwt is not None else 0, host_doubles(shift_lmn, 3),
        stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def dirty2ms_vis(uvw, freq, dirty, out, coef, pixsize_x, pixsize_y, epsilon=1e-7,
                 do_wstacking=True, flip_uw=False, dirty_strides=None, npix=None,
                 accumulate=False, shift_lmn=None, precision=None):
    """One image pol of predict_ng with the pol conversion fused into the
    write-back (sdp_hip_dirty2ms_vis): ``out`` [nrow, nchan, npol_vis] complex
    (any strides) gets coef[k] * predicted vis in pol k (coef None: pol 0)."""
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    npix_x, npix_y, dirty_strides = _dirty_in(dirty, dirty_strides, npix, 2)
    _check_vis(out, nrow, nchan, 3, "out")
    npv = out.shape[2]
    cbuf = _coef_buffer(coef, None, npv)
    bits = _flag_bits(flip_uw, accumulate, pbits)
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_dirty2ms_vis", *_uvw_args(uvw, freq, nchan, nrow),
              ptr(dirty), int(dirty_strides[0]), int(dirty_strides[1]),
              *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
              *_strided_args(out, 3, None), npv, cbuf, host_doubles(shift_lmn, 3), stream(dev),
              ctypes.byref(info))
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
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    npix_x, npix_y, dirty_strides = _dirty_in(dirty, dirty_strides, npix, 3)
    npo = dirty.shape[0]
    _check_vis(out, nrow, nchan, 3, "out")
    npv = out.shape[2]
    if not 1 <= npo <= 4:
        raise ValueError("npol_img must be 1..4")
    cbuf = _coef_buffer(coef, npo, npv)
    bits = _flag_bits(flip_uw, accumulate, pbits)
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_dirty2ms_vis_pols", *_uvw_args(uvw, freq, nchan, nrow),
              ptr(dirty), int(dirty_strides[1]), int(dirty_strides[2]), int(dirty_strides[0]), npo,
              *_grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking, bits),
              *_strided_args(out, 3, None), npv, cbuf, host_doubles(shift_lmn, 3), stream(dev),
              ctypes.byref(info))
    return out, info.as_dict()


def dirty2ms(uvw, freq, dirty, wgt, pixsize_x, pixsize_y, epsilon=1e-7,
             do_wstacking=True, flip_uw=False, out=None, dirty_strides=None,
             npix=None, accumulate=False, vis_dtype=torch.complex64, precision=None):
    """ducc0.wgridder.dirty2ms semantics on device; returns vis [nrow,nchan]."""
    dev, freq, nrow, nchan, pbits = _prologue(uvw, freq, epsilon, precision)
    npix_x, npix_y, dirty_strides = _dirty_in(dirty, dirty_strides, npix, 2)
    _check_wgt(wgt, nrow, nchan)
    if out is None:
        out = alloc((nrow, nchan), vis_dtype, dev)
    _check_vis(out, nrow, nchan, 2, "vis out")
    grid = _grid_args(npix_x, npix_y, pixsize_x, pixsize_y, epsilon, do_wstacking,
                      _flag_bits(flip_uw, accumulate, pbits))
    info = _lib.WGridInfo()
    _lib.call("sdp_hip_dirty2ms", *_uvw_args(uvw, freq, nchan, nrow),
              ptr(dirty), int(dirty_strides[0]), int(dirty_strides[1]), *grid[:4],
              *_strided_args(wgt, 2, _lib.SDP_HIP_F32), *grid[4:],
              *_strided_args(out, 2, None), stream(dev), ctypes.byref(info))
    return out, info.as_dict()


def set_stage_timing(enable):
    _lib.load().sdp_hip_set_stage_timing(int(bool(enable)))


def release_workspace():
    _lib.call("sdp_hip_release_workspace")
