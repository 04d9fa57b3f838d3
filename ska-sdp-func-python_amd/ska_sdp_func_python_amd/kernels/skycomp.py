"""Sky-component image operations (csrc/skycomp.hip): sdp_hip_skycomp_*."""

import torch

from .. import _lib
from ._operands import DT_CODE, dev_array, on_gpu, ptr, stream

# (tile, component) pairs listed per launch; a longer list is split by component
# range into several launches, which keeps every pixel's order of addition
# (making the list takes about ten int64 temporaries per pair on the device)
SKYCOMP_MAX_PAIRS = 1 << 24
# restore leaves a component out of a tile where the exponent's argument
# exceeds this on the whole tile: exp(-700) ~ 1e-304
RESTORE_SKIP_ARGUMENT = 700.0


def _skycomp_image(image):
    on_gpu(image, "image")
    if image.dim() != 4 or image.dtype not in (torch.float32, torch.float64) \
            or not image.is_contiguous():
        raise ValueError("image must be a contiguous float32 or float64 device tensor "
                         "[nchan, npol, ny, nx]")
    nchan, npol, ny, nx = image.shape
    if ny * nx >= 2 ** 31:
        raise ValueError("image planes of 2^31 pixels or more are not supported")
    return nchan * npol, ny, nx


def tile_boxes(x_lo, x_hi, y_lo, y_hi, ny, nx):
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


def tile_csr(boxes, start, stop, ny, nx, dev):
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
    tile_ptr = torch.searchsorted(tile, torch.arange(ntiles + 1, device=dev))
    return tile_ptr, comp[order].to(torch.int32)


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
    boxes = tile_boxes(origin[:, 0], origin[:, 0] + L - 1, origin[:, 1], origin[:, 1] + L - 1,
                       ny, nx)
    for s, e in _skycomp_launches(boxes, ncomp):
        if not boxes[3][s:e].any():
            continue
        args = [dev_array(a, dt, dev) for a, dt in (
            (origin[s:e], np.int32), (taps_y[s:e], np.float64), (taps_x[s:e], np.float64),
            (insertsum[s:e], np.float64), (flux[s:e], np.float64))]
        args += tile_csr(boxes, s, e, ny, nx, dev)
        _lib.call("sdp_hip_skycomp_insert", nplanes, ny, nx, ptr(image), DT_CODE[image.dtype],
                  e - s, L, *[ptr(a) for a in args], stream(dev))
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
    boxes = tile_boxes(np.floor(xy[:, 0] - r), np.ceil(xy[:, 0] + r),
                       np.floor(xy[:, 1] - r), np.ceil(xy[:, 1] + r), ny, nx)
    dev = image.device
    for s, e in _skycomp_launches(boxes, ncomp):
        if not boxes[3][s:e].any():
            continue
        xy_d, flux_d = dev_array(xy[s:e], np.float64, dev), dev_array(flux[s:e], np.float64, dev)
        tile_ptr, comp = tile_csr(boxes, s, e, ny, nx, dev)
        _lib.call("sdp_hip_skycomp_restore", nplanes, ny, nx, ptr(image), DT_CODE[image.dtype],
                  e - s, ptr(xy_d), ptr(flux_d), a, b, c, ptr(tile_ptr), ptr(comp), stream(dev))
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
    pts = dev_array(xy, np.float64, dev)
    on_gpu(pts, "points")
    labels = torch.empty((ny, nx), dtype=torch.int64, device=dev)
    _lib.call("sdp_hip_skycomp_nearest", int(ny), int(nx), xy.shape[0], ptr(pts), ptr(labels),
              stream(dev))
    return labels
