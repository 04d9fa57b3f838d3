"""Bandpass resampling (csrc/bandpass.hip): sdp_hip_resample_polyfit / _interp."""

import torch

from .. import _lib
from ._operands import alloc, on_gpu, ptr, stream

BANDPASS_MAX_DEGREE = _lib.SDP_HIP_BANDPASS_MAX_DEGREE
BANDPASS_MAX_SEGMENTS = _lib.SDP_HIP_BANDPASS_MAX_SEGMENTS


def _bandpass_gain(gain):
    """(rows, c_in, nrec) of a gain table [T, A, C_in, R, R] complex128 on the device."""
    on_gpu(gain, "gain")
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
    out = alloc(tuple(gain.shape[:2]) + (c_out, nrec, nrec), torch.complex128, dev)
    tabs = [torch.as_tensor(a, device=dev) for a in (q, e, seg, edges)]
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_resample_polyfit", nrows, c_in, c_out, nrec, nd - 1, nseg, ptr(gain),
                  ptr(out), *[ptr(t) for t in tabs], stream(dev))
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
    out = alloc(tuple(gain.shape[:2]) + (c_out, nrec, nrec), torch.complex128, dev)
    tabs = [torch.as_tensor(a, device=dev) for a in (x_in, x_out, interval)]
    with torch.cuda.device(dev):
        _lib.call("sdp_hip_resample_interp", nrows, c_in, c_out, nrec, ptr(gain), ptr(out),
                  *[ptr(t) for t in tabs], stream(dev))
    return out
