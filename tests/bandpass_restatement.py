"""Restatements for the bandpass resamplers (csrc/bandpass.hip and
calibration/beamformer_utils.py), independent of the package's own tables.

The tight restatement of ``polyfit``: the least-squares polynomial per
segment, fitted in the centred variable t = (f - mid) / half-width, in
longdouble, by Householder QR of the Vandermonde matrix -- as a dense
operator M [C_out, C_in], so that both the fitted values (M g) and the
rounding bound of a computed one (sum_c |M[co, c]| |g_c|) can be read off it.
The reference's own fit in raw Hz is off this by about cond * eps; the
fixtures store that distance per case (S_case).

``polyfit_apply`` and ``interp_apply`` restate the two kernels in fp64 numpy
from the same host tables the kernels take (tests/test_beamformer_cpu.py puts
them in the kernel wrappers' place); ``interp_apply`` follows numpy's
arr_interp_complex operation by operation, so it is numpy.interp bit for bit.
"""

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def normalise_edges(edges, nfrequency):
    """The reference's set_edges (beamformer_utils.py:361-379)."""
    if edges is None or len(edges) == 0:
        edges = [0, nfrequency]
    edges = [int(v) for v in edges]
    if edges[0] > 0:
        edges = [0] + edges
    if edges[-1] < nfrequency:
        edges = edges + [nfrequency]
    return edges


def segments(freq_out, freq_in, edges):
    """seg [C_out]: the reference's sequential assignment (:411-417), the last
    matching segment wins; -1 where none matches."""
    freq_out, freq_in = np.asarray(freq_out, float), np.asarray(freq_in, float)
    seg = np.full(len(freq_out), -1)
    dfreq = freq_in[1] - freq_in[0]
    for k in range(len(edges) - 1):
        seg[(freq_out >= freq_in[edges[k]] - dfreq / 2)
            & (freq_out < freq_in[edges[k + 1] - 1] + dfreq / 2)] = k
    return seg


def _householder_lstsq_operator(v, v_out):
    """v_out @ pinv(v) for a full-rank tall v, by Householder QR in longdouble."""
    n, m = v.shape
    r = v.copy()
    qt = np.eye(n, dtype=LD)                  # accumulates Q^T
    for k in range(m):
        x = r[k:, k].copy()
        alpha = -np.copysign(np.sqrt(np.sum(x * x)), x[0])
        x[0] -= alpha
        norm = np.sqrt(np.sum(x * x))
        if norm == 0:
            continue
        w = x / norm
        r[k:, :] -= 2 * np.outer(w, w @ r[k:, :])
        qt[k:, :] -= 2 * np.outer(w, w @ qt[k:, :])
    # solve R c = Q^T[:m] for the coefficient operator [m, n] by back substitution
    coef = np.zeros((m, n), dtype=LD)
    for i in range(m - 1, -1, -1):
        coef[i] = (qt[i] - r[i, i + 1:m] @ coef[i + 1:]) / r[i, i]
    return v_out @ coef


def tight_operator(freq_out, freq_in, edges, polydeg):
    """(M [C_out, C_in] longdouble, seg): out = M g is the least-squares fit
    of degree ``polydeg`` per segment; rows of output channels in no segment
    are zero (their result is NaN, see ``apply_operator``)."""
    freq_out, freq_in = np.asarray(freq_out, float), np.asarray(freq_in, float)
    edges = normalise_edges(edges, len(freq_in))
    seg = segments(freq_out, freq_in, edges)
    m = np.zeros((len(freq_out), len(freq_in)), dtype=LD)
    powers = np.arange(polydeg + 1)
    for k in range(len(edges) - 1):
        lo, hi = edges[k], edges[k + 1]
        f = freq_in[lo:hi].astype(LD)
        mid, half = (f.max() + f.min()) / 2, (f.max() - f.min()) / 2
        half = half if half > 0 else LD(1)
        t = (f - mid) / half
        t_out = (freq_out[seg == k].astype(LD) - mid) / half
        m[np.ix_(seg == k, np.arange(lo, hi))] = _householder_lstsq_operator(
            t[:, None] ** powers, t_out[:, None] ** powers)
    return m, seg


def apply_operator(m, gain, seg=None):
    """M applied along the channel axis of gain [T, A, C_in, R, R] in
    longdouble, rounded to complex128; NaN + NaN j where seg is -1."""
    gain = np.asarray(gain)
    re = np.einsum("oc,tacij->taoij", m, gain.real.astype(LD))
    im = np.einsum("oc,tacij->taoij", m, gain.imag.astype(LD))
    out = re.astype(np.float64) + 1j * im.astype(np.float64)
    if seg is not None:
        out[:, :, np.asarray(seg) < 0] = np.nan + 1j * np.nan
    return out


def operator_scale(m, gain):
    """sum_c |M[co, c]| |g_c| per output element [T, A, C_out, R, R]: what the
    rounding bound of a computed M g is proportional to."""
    return np.einsum("oc,tacij->taoij", np.abs(np.asarray(m, dtype=np.float64)),
                     np.abs(np.asarray(gain)))


def polyfit_apply(gain, q, e, seg, edges):
    """The kernel sdp_hip_resample_polyfit in fp64 numpy (the sums in numpy's
    order, not the kernel's): [T, A, C_out, R, R] complex128."""
    gain = np.asarray(gain, dtype=np.complex128)
    q, e = np.asarray(q, float), np.asarray(e, float)
    seg, edges = np.asarray(seg), np.asarray(edges)
    out = np.full(gain.shape[:2] + (len(seg),) + gain.shape[3:], np.nan + 1j * np.nan)
    for k in range(len(edges) - 1):
        lo, hi = edges[k], edges[k + 1]
        coef = np.einsum("dc,tacij->tadij", q[:, lo:hi], gain[:, :, lo:hi])
        out[:, :, seg == k] = np.einsum("od,tadij->taoij", e[seg == k], coef)
    return out


def _interp_component(y, x_in, x_out, interval):
    """One real component y [..., C_in] -> [..., C_out], numpy's arithmetic."""
    c_in = len(x_in)
    j = np.clip(interval, 0, max(c_in - 2, 0))
    with np.errstate(all="ignore"):
        if c_in > 1:
            y0, y1 = y[..., j], y[..., j + 1]
            x0, x1 = x_in[j], x_in[j + 1]
            slope = (y1 - y0) * (1.0 / (x1 - x0))
            r = slope * (x_out - x0) + y0
            bad = np.isnan(r)
            r2 = slope * (x_out - x1) + y1
            r = np.where(bad, r2, r)
            r = np.where(bad & np.isnan(r2) & (y0 == y1), y0, r)
            r = np.where(x0 == x_out, y0, r)
        else:
            r = np.repeat(y[..., :1], len(x_out), axis=-1)
    r = np.where(interval == -1, y[..., :1], r)
    r = np.where(interval >= c_in - 1, y[..., -1:], r)
    return r


def interp_apply(gain, x_in, x_out, interval):
    """The kernel sdp_hip_resample_interp in fp64 numpy: numpy.interp along
    the channel axis of gain [T, A, C_in, R, R], bit for bit."""
    gain = np.asarray(gain, dtype=np.complex128)
    x_in, x_out = np.asarray(x_in, float), np.asarray(x_out, float)
    interval = np.asarray(interval)
    g = np.moveaxis(gain, 2, -1)
    re = _interp_component(g.real, x_in, x_out, interval)
    im = _interp_component(g.imag, x_in, x_out, interval)
    nan = interval == -2
    re = np.where(nan, x_out, re)
    im = np.where(nan, 0.0, im)
    out = np.empty(re.shape, dtype=np.complex128)   # not re + 1j * im: a NaN part stays its own
    out.real, out.imag = re, im
    return np.ascontiguousarray(np.moveaxis(out, -1, 2))


def spline_apply(op, gain):
    """The dense spline operator [C_out, C_in] applied along the channel axis."""
    return np.einsum("oc,tacij->taoij", np.asarray(op), np.asarray(gain))


def reference_condition(freq_in, edges, polydeg):
    """Per segment (smallest / largest singular value, rcond) of the scaled
    Vandermonde matrix numpy.polynomial.polyfit decomposes: columns f^k in raw
    Hz, each divided by its 2-norm; rcond = n * eps."""
    freq_in = np.asarray(freq_in, float)
    edges = normalise_edges(edges, len(freq_in))
    out = []
    for k in range(len(edges) - 1):
        f = freq_in[edges[k]:edges[k + 1]]
        van = np.polynomial.polynomial.polyvander(f, polydeg)
        van = van / np.sqrt(np.square(van).sum(0))
        s = np.linalg.svd(van, compute_uv=False)
        out.append((float(s[-1] / s[0]), len(f) * EPS))
    return out
