"""ctypes binding of libska_sdp_hip.so (the C ABI declared in include/ska_sdp_hip.h).

The product path has exactly one backend: the hand-written HIP kernels in this
library.  If the shared object is missing or no GPU is visible, every compute
entry point raises -- there is deliberately no CPU fallback.
"""

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDP_HIP_LIB_OVERRIDE: load another build of the same C ABI (kernel-variant
# experiments, scripts/build_variants.sh); the default is the in-tree build.
LIB_PATH = os.environ.get("SDP_HIP_LIB_OVERRIDE") or os.path.join(_HERE, "_lib", "libska_sdp_hip.so")

SDP_HIP_OK = 0
SDP_HIP_ERR_INVALID_ARG = 1
SDP_HIP_ERR_RUNTIME = 2
SDP_HIP_ERR_NO_DEVICE = 3
SDP_HIP_ERR_MEMORY = 4

SDP_HIP_F32 = 1
SDP_HIP_F64 = 2
SDP_HIP_C64 = 3
SDP_HIP_C128 = 4

SDP_HIP_FLIP_UW = 1
SDP_HIP_ACCUMULATE = 2
SDP_HIP_BATCH_FIRST = 4
SDP_HIP_BATCH_LAST = 8
SDP_HIP_KEEP_BUCKETS = 16
SDP_HIP_REUSE_BUCKETS = 32
SDP_HIP_FP32 = 64
SDP_HIP_W_SLAB = 128
SDP_HIP_SLOT1 = 256

SDP_HIP_CLEAN_HOGBOM = 0
SDP_HIP_CLEAN_MSCLEAN = 1
SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL = 0
SDP_HIP_MFSCLEAN_FINDPEAK_CASA = 1
SDP_HIP_STOKES_IQUV = 0
SDP_HIP_STOKES_I = 1
SDP_HIP_SKYCOMP_TILE_X = 32
SDP_HIP_SKYCOMP_TILE_Y = 8
SDP_HIP_MIX_PLANES_REGS = 8
SDP_HIP_MIX_PLANES_MAX = 4096
SDP_HIP_MIX_NAN_INPUT = 1
SDP_HIP_MIX_NAN_OUTPUT = 2
SDP_HIP_GATHER_FACETS_MAX = 256
SDP_HIP_SEGMENT_TILE = 32
SDP_HIP_SEGMENT_KERNEL_MAX = 15
SDP_HIP_GAIN_CHAIN_MAX = 8
SDP_HIP_GAUSS_FIT_WINDOW = 15
SDP_HIP_BANDPASS_MAX_DEGREE = 7
SDP_HIP_BANDPASS_MAX_SEGMENTS = 64
SDP_HIP_SUM_PLANES_MAX = 4096
SDP_HIP_PEAK_MOMENT0 = 0
SDP_HIP_PEAK_REFCHAN = 1
SDP_HIP_PEAK_NAN_INPUT = 1
SDP_HIP_PEAK_NAN_MEAN = 2

c_i64 = ctypes.c_int64
c_int = ctypes.c_int
c_dbl = ctypes.c_double
c_vp = ctypes.c_void_p
c_u32 = ctypes.c_uint
c_size = ctypes.c_size_t
c_char_p = ctypes.c_char_p


class WGridInfo(ctypes.Structure):
    _fields_ = [
        ("support", c_int),
        ("beta", c_dbl),
        ("ngrid_x", c_int),
        ("ngrid_y", c_int),
        ("nplanes", c_int),
        ("w0", c_dbl),
        ("dw", c_dbl),
        ("nvis_used", c_i64),
        ("nitems", c_i64),
        ("plane_chunk", c_int),
        ("ms_prep", ctypes.c_float),
        ("ms_grid", ctypes.c_float),
        ("ms_fft", ctypes.c_float),
        ("ms_screen", ctypes.c_float),
        ("bucket", c_int),
        ("grid_launches", c_int),
        ("padded", c_int),
        ("fp64", c_int),
        ("tiled", c_int),
        ("folded", c_int),
        ("layout_reused", c_int),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# (symbol, argtypes) for every entry point declared in include/ska_sdp_hip.h
_ERR = [c_char_p, c_size]
SIGNATURES = {
    "sdp_hip_version": [],
    "sdp_hip_device_count": [ctypes.POINTER(c_int)] + _ERR,
    "sdp_hip_release_workspace": _ERR,
    "sdp_hip_set_stage_timing": [c_int],
    "sdp_hip_ms2dirty": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_int, c_i64, c_i64,                # vis, dtype, strides
        c_vp, c_int, c_i64, c_i64,                # wgt, dtype (f32 / f64), strides
        c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_u32,
        c_vp, c_i64, c_i64,                       # dirty, strides
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_ms2dirty_batch": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_int, c_i64, c_i64,                # vis, dtype, strides
        c_vp, c_int, c_i64, c_i64,                # wgt, dtype (f32 / f64), strides
        c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_u32,
        c_vp,                                     # bounds (host, 6 doubles; 8 with W_SLAB)
        c_vp, c_i64, c_i64,                       # dirty, strides
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_wstack_layout": [
        c_vp, c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_u32,  # bounds, geometry, eps, do_w, flags
        ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_wstack_fingerprint": [c_vp, c_i64, c_i64, c_vp, c_int, c_vp] + _ERR,
    "sdp_hip_ms2dirty_vis": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # vis, dtype, row/chan/pol strides, npol_vis
        c_vp,                                     # pol_coeff (host doubles) or NULL
        c_vp, c_int, c_i64, c_i64,                # wgt, dtype, strides
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # flags, bytes, strides, pol
        c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_u32,
        c_vp, c_i64, c_i64, c_vp,                 # dirty, strides, sumwt
        c_vp,                                     # shift_lmn (host doubles) or NULL
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_ms2dirty_vis_pols": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # vis, dtype, row/chan/pol strides, npol_vis
        c_vp, c_int,                              # pol_coeff (host doubles) or NULL, npol_img
        c_vp, c_int, c_i64, c_i64, c_i64,         # wgt, dtype, row/chan/pol strides
        c_vp, c_int, c_i64, c_i64, c_i64,         # flags, bytes, strides
        c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_u32,
        c_vp, c_i64, c_i64, c_i64,                # dirty, x / y / pol strides
        c_vp, c_i64,                              # sumwt, its pol stride
        c_vp,                                     # shift_lmn (host doubles) or NULL
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_ms2dirty_vis_batch": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # vis, dtype, row/chan/pol strides, npol_vis
        c_vp,                                     # pol_coeff (host doubles) or NULL
        c_vp, c_int, c_i64, c_i64,                # wgt, dtype, strides
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # flags, bytes, strides, pol
        c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_u32,
        c_vp,                                     # bounds (host, 6 doubles)
        c_vp, c_i64, c_i64, c_vp,                 # dirty, strides, sumwt
        c_vp,                                     # shift_lmn (host doubles) or NULL
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_dirty2ms": [
        c_vp, c_i64, c_vp, c_int, c_i64,
        c_vp, c_i64, c_i64, c_int, c_int, c_dbl, c_dbl,
        c_vp, c_int, c_i64, c_i64,                # wgt, dtype (f32 / f64), strides
        c_dbl, c_int, c_u32,
        c_vp, c_int, c_i64, c_i64,
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_dirty2ms_vis": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_i64, c_i64, c_int, c_int, c_dbl, c_dbl,
        c_dbl, c_int, c_u32,
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # vis, dtype, strides, npol_vis
        c_vp,                                     # pol_coeff (host doubles) or NULL
        c_vp,                                     # shift_lmn (host doubles) or NULL
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_dirty2ms_vis_pols": [
        c_vp, c_i64, c_vp, c_int, c_i64,          # uvw, stride, freq, nchan, nrow
        c_vp, c_i64, c_i64, c_i64, c_int,         # dirty, x / y / pol strides, npol_img
        c_int, c_int, c_dbl, c_dbl,
        c_dbl, c_int, c_u32,
        c_vp, c_int, c_i64, c_i64, c_i64, c_int,  # vis, dtype, strides, npol_vis
        c_vp,                                     # pol_coeff [npol_img][npol_vis] or NULL
        c_vp,                                     # shift_lmn (host doubles) or NULL
        c_vp, ctypes.POINTER(WGridInfo)] + _ERR,
    "sdp_hip_dft_point_v00": [
        c_int, c_vp, c_vp, c_int, c_int, c_i64, c_int, c_vp, c_vp, c_int, c_vp] + _ERR,
    "sdp_hip_dft_point_metres": [
        c_int, c_vp, c_vp, c_int, c_int, c_i64, c_int, c_vp, c_vp, c_vp, c_int,
        c_vp] + _ERR,
    "sdp_hip_idft_point_v00": [
        c_int, c_vp, c_int, c_i64, c_int, c_vp,   # ncomp, dc, npol, nrow, nchan, uvw_lambda
        c_vp, c_int, c_vp, c_vp, c_int,           # vis, dtype, weight, flags, flag_bytes
        c_vp, c_vp, c_vp] + _ERR,                 # flux_sum, sumwt, stream
    "sdp_hip_idft_point_metres": [
        c_int, c_vp, c_int, c_i64, c_int, c_vp, c_vp,  # ..., uvw (metres), freq
        c_vp, c_int, c_vp, c_vp, c_int,
        c_vp, c_vp, c_vp] + _ERR,
    "sdp_hip_grid_cf": [
        c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
        c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int,
        c_int, c_vp, c_vp, c_vp] + _ERR,
    "sdp_hip_degrid_cf": [
        c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
        c_int, c_int, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
        c_vp, c_vp] + _ERR,
    "sdp_hip_solve_gains": [
        c_int, c_int, c_int, c_vp, c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp,
        c_vp, c_vp, c_int, c_dbl, c_int, c_int, c_dbl, c_vp] + _ERR,
    "sdp_hip_point_sums": [
        c_i64, c_int, c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp,
        c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp] + _ERR,
    "sdp_hip_divide_vis": [
        c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp] + _ERR,
    "sdp_hip_apply_gains": [
        c_i64, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_int, c_int, c_vp, c_vp, c_vp,
        c_vp, c_int, c_int, c_int, c_int, c_int, c_vp] + _ERR,
    "sdp_hip_apply_gain_chain": [
        c_i64, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp,  # shape, vis, dtype, weight, ants
        c_int, c_int, c_vp, c_vp,                 # nants, ntab, gains (host), time_rows (host)
        c_vp, c_vp, c_vp, c_int, c_vp] + _ERR,    # nrow_g, nchan_g, nrec (host), inverse, stream
    "sdp_hip_grid_weights": [
        c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int,
        c_int, c_vp, c_vp, c_vp] + _ERR,
    "sdp_hip_reweight": [
        c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_int,
        c_int, c_int, c_dbl, c_vp, c_int, c_vp, c_vp] + _ERR,
    "sdp_hip_taper": [
        c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_dbl, c_vp, c_vp] + _ERR,
    "sdp_hip_clean_plane": [
        c_int, c_int, c_int, c_int, c_int, c_int,   # algorithm, nscales, ny, nx, psf_ny, psf_nx
        c_vp, c_vp, c_vp, c_vp,                     # res, psf, window, sensitivity
        c_vp, c_vp, c_int, c_vp,                    # coupling_diag (host), scale_kernels, extent, comps
        c_dbl, c_dbl, c_dbl, c_int,                 # gain, pmax, absthresh, niter
        ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp] + _ERR,
    "sdp_hip_clean_plane_complex": [
        c_int, c_int, c_int, c_int,                 # ny, nx, psf_ny, psf_nx
        c_vp, c_vp, c_vp, c_vp,                     # res [2, ny, nx], psf, window, comps [2, ny, nx]
        c_dbl, c_dbl, c_dbl, c_int,                 # gain, pmax, absthresh, niter
        ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp] + _ERR,
    "sdp_hip_mfsclean_plane": [
        c_int, c_int, c_int, c_int, c_int, c_int,   # nscales, nmoment, ny, nx, psf_ny, psf_nx
        c_vp, c_vp, c_vp, c_vp, c_int,              # smresidual, m_model, ssmmpsf, scale_kernels, extent
        c_vp, c_vp, c_vp, c_vp,                     # windowstack, sensitivity, hsmmpsf, ihsmmpsf (host)
        c_int, c_dbl, c_dbl, c_int,                 # findpeak, gain, absthresh, niter
        ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_vp, c_vp] + _ERR,  # done, reason, counts (host)
    "sdp_hip_vis_average_channels": [
        c_i64, c_int, c_int, c_int, c_int,        # nrows, nchan, npol, group, variant
        c_vp, c_int, c_vp, c_vp, c_vp, c_int,     # vis, dtype, weight, imaging_weight, flags, bytes
        c_vp, c_vp, c_vp, c_vp, c_int, c_vp] + _ERR,  # outputs, flags_out bytes, stream
    "sdp_hip_vis_to_stokes": [
        c_i64, c_int, c_int, c_vp, c_int,         # nsamples, npol, mode, vis, dtype
        c_vp, c_vp, c_vp, c_int, c_vp,            # weight, imaging_weight, flags, bytes, matrix (host)
        c_vp, c_vp, c_vp, c_vp, c_int, c_vp] + _ERR,  # outputs, flags_out bytes, stream
    "sdp_hip_vis_remove_continuum": [
        c_i64, c_int, c_int, c_vp, c_int,         # nrows, nchan, npol, vis, dtype
        c_vp, c_vp, c_int, c_vp, c_vp, c_int,     # weight, flags, bytes, x, mask, degree
        c_vp, c_int, c_vp, c_vp] + _ERR,          # rank_list, capacity, rank_count, stream
    "sdp_hip_skycomp_insert": [
        c_int, c_int, c_int, c_vp, c_int,         # nplanes, ny, nx, image, dtype
        c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp,  # ncomp, window, origin, taps y / x, sum, flux
        c_vp, c_vp, c_vp] + _ERR,                 # tile_ptr, tile_comp, stream
    "sdp_hip_skycomp_restore": [
        c_int, c_int, c_int, c_vp, c_int,         # nplanes, ny, nx, image, dtype
        c_i64, c_vp, c_vp, c_dbl, c_dbl, c_dbl,   # ncomp, xy, flux, a, b, c
        c_vp, c_vp, c_vp] + _ERR,                 # tile_ptr, tile_comp, stream
    "sdp_hip_skycomp_nearest": [
        c_int, c_int, c_i64, c_vp, c_vp, c_vp] + _ERR,  # ny, nx, ncomp, xy, labels, stream
    "sdp_hip_mix_planes": [
        c_int, c_int, c_i64, c_vp, c_int,         # nin, nout, npix, in_planes (host), dtype
        c_vp, c_vp, ctypes.POINTER(c_int), c_vp] + _ERR,  # out_planes, weights (host), nan_seen, stream
    "sdp_hip_gather_facets": [
        c_int, c_int, c_int, c_int, c_int,        # dtype, facets, nplanes, ny, nx
        c_int, c_int, c_int, c_int, c_int, c_int,  # dy, dx, y0, x0, sy, sx
        c_vp, c_vp, c_vp, c_vp, c_vp, c_int,      # facet tables, tapers (host), normalise
        c_vp, c_vp, c_vp] + _ERR,                 # out, sumwt, stream
    "sdp_hip_segment_label": [
        c_int, c_int, c_int, c_vp, c_int, c_i64,  # nchan, ny, nx, planes, dtype, plane stride
        c_int, c_vp, c_dbl, c_dbl,                # ksize, taps (host), tap_sum, threshold
        c_vp, c_vp, c_vp, c_vp] + _ERR,           # labels, count, nonfinite, stream
    "sdp_hip_segment_roots": [
        c_int, c_int, c_vp, c_vp, c_int, c_vp, c_vp] + _ERR,  # ny, nx, labels, count, npixels, keep
    "sdp_hip_segment_relabel": [
        c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp] + _ERR,  # ny, nx, labels, keep, rank, segmap
    "sdp_hip_segment_peaks": [
        c_int, c_int, c_int, c_vp, c_int, c_i64,  # nplanes, ny, nx, planes, dtype, plane stride
        c_vp, c_int, c_vp, c_vp, c_vp] + _ERR,    # segmap, nseg, values, indices, stream
    "sdp_hip_gauss_fit": [
        c_int, c_vp, c_int, c_vp, c_vp, c_vp,     # nfit, planes (host), dtype, strides, x0, y0 (host)
        c_int, c_vp, c_vp, c_vp, c_vp] + _ERR,    # max_iter, params, status, niter, stream
    "sdp_hip_resample_polyfit": [
        c_i64, c_int, c_int, c_int, c_int, c_int,  # nrows, c_in, c_out, nrec, degree, nseg
        c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp] + _ERR,  # gain, out, q, e, seg, edges, stream
    "sdp_hip_resample_interp": [
        c_i64, c_int, c_int, c_int,               # nrows, c_in, c_out, nrec
        c_vp, c_vp, c_vp, c_vp, c_vp, c_vp] + _ERR,  # gain, out, x_in, x_out, interval, stream
    "sdp_hip_sum_planes": [
        c_int, c_i64, c_i64, c_vp, c_int, c_vp,   # ncube, nplane, npix, in_cubes (host), dtype, out
        c_vp, c_vp, c_int, c_vp] + _ERR,          # weights, sumwt (device), normalise, stream
    "sdp_hip_peak_abs": [
        c_int, c_int, c_int, c_int, c_int,        # mode, nchan, npol, ny, nx
        c_vp, c_int, c_i64, c_i64, c_i64,         # cube, dtype, chan / pol / row strides
        ctypes.POINTER(c_dbl), ctypes.POINTER(c_int), c_vp] + _ERR,  # peak, nan_seen (host), stream
    "sdp_hip_wkernel_create": [
        c_int, c_int, c_int, c_int, c_int, c_dbl,  # npixel, oversampling, support, nw, npb, fov
        c_vp, c_vp, c_vp, c_vp, c_vp] + _ERR,     # w, taper, pb, cf, stream
}

_lock = threading.Lock()
_lib = None


class HipLibraryError(RuntimeError):
    """Raised when the native library is missing or no GPU is available."""


def load():
    """Load (once) and return the ctypes handle; raise if it is absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f"{LIB_PATH} not built: run __graft_entry__.build() "
                "(there is no CPU fallback for the HIP path)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is None:
                continue
            fn.argtypes = argtypes
            fn.restype = c_int
        _lib = lib
        return lib


def exported_symbols():
    lib = load()
    return [name for name in SIGNATURES if hasattr(lib, name)]


def errbuf():
    return ctypes.create_string_buffer(1024)


def check(status, buf):
    if status == SDP_HIP_OK:
        return
    msg = buf.value.decode(errors="replace") if buf is not None else ""
    if status == SDP_HIP_ERR_INVALID_ARG:
        raise ValueError(msg)
    if status == SDP_HIP_ERR_MEMORY:
        raise MemoryError(msg)
    raise RuntimeError(msg or f"libska_sdp_hip status {status}")


def call(name, *args):
    fn = getattr(load(), name)
    buf = errbuf()
    status = fn(*args, buf, ctypes.sizeof(buf))
    check(status, buf)
