"""CLEAN minor cycles (csrc/clean.hip, csrc/mfsclean.hip)."""

import ctypes

import torch

from .. import _lib
from ._operands import host_doubles, on_gpu, ptr, stream

CLEAN_STOP = {0: "niter", 1: "threshold", 2: "zero"}


def _f64_plane(t, name, shape):
    on_gpu(t, name)
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
    on_gpu(res, "res")
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
              pnx, ptr(res), ptr(psf), ptr(window), ptr(sensitivity), cd,
              ptr(scale_kernels if ms else None), int(scale_extent), ptr(comps), float(gain),
              float(pmax), float(absthresh), int(niter),
              ctypes.byref(done), ctypes.byref(reason), stream(res.device))
    return done.value, CLEAN_STOP[reason.value]


def clean_plane_complex(res, psf, comps, gain, pmax, absthresh, niter, window=None):
    """Up to ``niter`` complex Hogbom minor cycles of a Q / U pair cleaned as
    Q + iU, in place on device f64: ``res`` [2, ny, nx] (plane 0 Q, plane 1 U),
    ``psf`` [py, px] shared by both, ``comps`` [2, ny, nx]; optional ``window``
    [ny, nx].  The peak is the first maximum of hypot(q * w, u * w), the
    component (res[:, peak] * gain) * (1 / pmax), and the cycles stop once
    hypot(q, u) at the peak is below ``absthresh`` after the subtraction.
    Returns (cycles run, "niter" | "threshold")."""
    on_gpu(res, "res")
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
    _lib.call("sdp_hip_clean_plane_complex", ny, nx, pny, pnx, ptr(res), ptr(psf), ptr(window),
              ptr(comps), float(gain), float(pmax), float(absthresh), int(niter),
              ctypes.byref(done), ctypes.byref(reason), stream(res.device))
    return done.value, CLEAN_STOP[reason.value]


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
    on_gpu(smresidual, "smresidual")
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
        hess.append(host_doubles(flat))
    casa = findpeak == "CASA"
    done, reason = ctypes.c_int(0), ctypes.c_int(0)
    counts = (ctypes.c_int * ns)()
    _lib.call("sdp_hip_mfsclean_plane", ns, nt, ny, nx, pny, pnx, ptr(smresidual), ptr(m_model),
              ptr(ssmmpsf), ptr(scale_kernels), int(scale_extent), ptr(windowstack),
              ptr(sensitivity), hess[0], hess[1],
              _lib.SDP_HIP_MFSCLEAN_FINDPEAK_CASA if casa else _lib.SDP_HIP_MFSCLEAN_FINDPEAK_RASCIL,
              float(gain), float(absthresh), int(niter), ctypes.byref(done), ctypes.byref(reason),
              ctypes.cast(counts, ctypes.c_void_p), stream(smresidual.device))
    return done.value, CLEAN_STOP[reason.value], list(counts)
