"""Convolution-function gridding and degridding (csrc/cfgrid.hip)."""

import torch

from .. import _lib
from ._operands import ptr, stream


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


def _map_args(maps):
    return [ptr(maps[k]) for k in ("pu", "pv", "pwc", "pdu", "pdv")]


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
    _lib.call("sdp_hip_grid_cf", nrow, nchan, npol, *_map_args(maps), ptr(v2i), ptr(vis),
              ptr(wt), ptr(cf), cfn, nw, ndv, ndu, gv, gu, ptr(grid), gn, ny, nx, ptr(sumwt),
              ptr(skipped), stream(vis.device))
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
    _lib.call("sdp_hip_degrid_cf", nrow, nchan, npol, *_map_args(maps), ptr(v2i),
              ptr(grid), gn, ny, nx, ptr(cf), cfn, nw, ndv, ndu, gv, gu, ptr(out),
              ptr(skipped), stream(grid.device))
    return skipped
