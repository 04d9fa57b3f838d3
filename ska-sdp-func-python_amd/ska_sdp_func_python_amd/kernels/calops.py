"""Calibration (csrc/stefcal.hip, csrc/calops.hip): StefCal and its
neighbours sdp_hip_point_sums / divide_vis / apply_gains / apply_gain_chain."""

import ctypes

import torch

from .. import _lib
from ._operands import DT_CODE, f64_like, flags_of, on_gpu, ptr, ptr_table, stream, vis4

GAIN_CHAIN_MAX = _lib.SDP_HIP_GAIN_CHAIN_MAX


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
    xb = on_gpu(xb, "xb").to(torch.complex128).contiguous()
    wb = on_gpu(wb, "wb").to(torch.float64).contiguous()
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
    _lib.call("sdp_hip_solve_gains", nsolve, nants, nbl, ptr(rs), ptr(a2), nchan, npol,
              int(mode), ptr(xb), ptr(wb), ptr(gain), ptr(gwt), ptr(residual), ptr(used),
              int(niter), float(tol), int(bool(phase_only)), int(refant), float(damping),
              stream(xb.device))
    return residual, used


def _model_flags(model_flags, fl):
    """The model's own flags in the vis flags' dtype, or None."""
    if model_flags is None or fl is None:
        return None
    on_gpu(model_flags, "model_flags")
    if model_flags.shape != fl.shape:
        raise ValueError("model flags must be shaped like vis")
    return model_flags.to(fl.dtype).contiguous()


def point_sums(vis, model, weight, flags, row_ptr, time_idx, nchan_g, perm=None, conj=None,
               model_flags=None):
    """x_b, xwt_b [nrow_g, nbl, nchan_g, npol] (c128, f64) of solve_gaintable
    over divide_visibility(vis, model) (model None: vis itself)."""
    vis4(vis, "vis")
    if model is not None:
        vis4(model, "model")
        if model.shape != vis.shape or model.dtype != vis.dtype:
            raise ValueError("model must match vis")
    nt, nbl, nchan, npol = vis.shape
    if weight is not None:
        f64_like(weight, "weight", vis)
    fl, fb = flags_of(flags, vis.shape)
    nrow_g = row_ptr.numel() - 1
    nout = nbl if perm is None else perm.numel()
    if perm is not None and (perm.dtype != torch.int32 or (conj is not None and (
            conj.dtype != torch.uint8 or conj.numel() != nout))):
        raise ValueError("perm must be int32 and conj uint8 of the same length")
    xb = torch.empty((nrow_g, nout, nchan_g, npol), dtype=torch.complex128, device=vis.device)
    xwt = torch.empty((nrow_g, nout, nchan_g, npol), dtype=torch.float64, device=vis.device)
    mfl = _model_flags(model_flags, fl)
    _lib.call("sdp_hip_point_sums", nt, nbl, nchan, npol, ptr(vis), ptr(model),
              DT_CODE[vis.dtype], ptr(weight), ptr(fl), ptr(mfl), fb, nrow_g, ptr(row_ptr),
              ptr(time_idx), int(nchan_g), int(nout), ptr(perm), ptr(conj), ptr(xb),
              ptr(xwt), stream(vis.device))
    return xb, xwt


def divide_vis(vis, model, weight, flags, model_flags=None):
    """(x, xwt) of divide_visibility, same shapes as vis."""
    vis4(vis, "vis")
    vis4(model, "model")
    if model.shape != vis.shape or model.dtype != vis.dtype:
        raise ValueError("model must match vis")
    fl, fb = flags_of(flags, vis.shape)
    x = torch.empty_like(vis)
    xwt = torch.empty(vis.shape, dtype=torch.float64, device=vis.device)
    mfl = _model_flags(model_flags, fl)
    _lib.call("sdp_hip_divide_vis", vis.numel(), ptr(vis), ptr(model), DT_CODE[vis.dtype],
              ptr(weight), ptr(fl), ptr(mfl), fb, ptr(x), ptr(xwt), stream(vis.device))
    return x, xwt


def apply_gains(vis, weight, flags, use_flags, ant1, ant2, time_row, gain, inverse):
    """apply_gaintable in place on device vis / weight [t, b, f, p]."""
    vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    f64_like(weight, "weight", vis)
    fl, fb = flags_of(flags, vis.shape)
    on_gpu(gain, "gain")
    if gain.dtype != torch.complex128 or gain.dim() != 5 or not gain.is_contiguous():
        raise ValueError("gain must be contiguous complex128 [rows, nants, nchan, nrec, nrec]")
    nrow_g, nants, nchan_g, nrec, _ = gain.shape
    _lib.call("sdp_hip_apply_gains", nt, nbl, nchan, npol, ptr(vis), DT_CODE[vis.dtype],
              ptr(weight), ptr(fl), fb, int(bool(use_flags)), ptr(ant1), ptr(ant2),
              ptr(time_row), ptr(gain), nrow_g, nants, nchan_g, nrec, int(bool(inverse)),
              stream(vis.device))
    return vis, weight


def apply_gain_chain(vis, weight, ant1, ant2, time_rows, gains, inverse):
    """The gain tables ``gains`` (each complex128 [rows, nants, nchan_g, nrec,
    nrec]) with their time-row maps ``time_rows`` (each int32 [ntimes], -1 =
    no row) applied in order, in place on device vis / weight [t, b, f, p]:
    bit for bit what one ``apply_gains(..., use_flags=False)`` per table
    gives, in one pass over vis and weight per group of up to
    ``GAIN_CHAIN_MAX`` tables (sdp_hip_apply_gain_chain)."""
    vis4(vis, "vis")
    nt, nbl, nchan, npol = vis.shape
    f64_like(weight, "weight", vis)
    gains, time_rows = list(gains), list(time_rows)
    if len(gains) != len(time_rows):
        raise ValueError("one time_row map per gain table")
    for a in (ant1, ant2):
        on_gpu(a, "ant1 / ant2")
        if a.dtype != torch.int32 or a.numel() != nbl or not a.is_contiguous():
            raise ValueError("ant1 / ant2 must be contiguous int32 [nbl]")
    nants = gains[0].shape[1] if gains and gains[0].dim() == 5 else 1
    for g, tr in zip(gains, time_rows):
        on_gpu(g, "gain")
        on_gpu(tr, "time_row")
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
        _lib.call("sdp_hip_apply_gain_chain", nt, nbl, nchan, npol, ptr(vis),
                  DT_CODE[vis.dtype], ptr(weight), ptr(ant1), ptr(ant2), int(nants), n,
                  ptr_table(gs), ptr_table(trs),
                  (i32 * (n + 1))(*[g.shape[0] for g in gs]),
                  (i32 * (n + 1))(*[g.shape[2] for g in gs]),
                  (i32 * (n + 1))(*[g.shape[3] for g in gs]), int(bool(inverse)),
                  stream(vis.device))
    return vis, weight
