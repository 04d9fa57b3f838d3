"""grid_visibility_to_griddata / degrid_visibility_from_griddata on MI355X.

Mirrors reference ``src/ska_sdp_func_python/grid_data/gridding.py``:

* ``spatial_mapping`` (:60-157): nearest grid point through the grid WCS,
  sub-sample offsets through cf_wcs axes 3-4, nearest w plane through cf_wcs
  axis 5, with the reference's range assertions (numpy's round-half-even,
  reproduced by torch.round).  Evaluated in fp64 on the device.
* ``grid_visibility_to_griddata`` (:160-255): conj(CF) * vis * weight added
  per visibility into the GridData with the edge-skip rule (:230-237),
  ``sumwt`` over the non-skipped rows; the per-row slice adds run in the HIP
  kernel sdp_hip_grid_cf (fp64 atomics).
* ``degrid_visibility_from_griddata`` (:502-590): einsum("ij,ij") of the grid
  window with the CF, in sdp_hip_degrid_cf.
* ``grid_visibility_weight_to_griddata`` (:258-334) and
  ``griddata_visibility_reweight`` (:362-499): imaging weights in
  sdp_hip_grid_weights / sdp_hip_reweight (same nearest-cell mapping and
  skip rules; fp64 atomics), ``griddata_merge_weights`` (:337-359).
* ``fft_griddata_to_image`` / ``fft_image_to_griddata`` (:593-645): centred
  2-D FFTs (reference fft_support.py:31-140) via rocFFT (torch.fft on the
  HIP device), times nx*ny on the inverse, with the optional gcf.
"""

import copy
import logging

import numpy as np
import torch

from .. import _device, kernels
from ..datamodels import Image

log = logging.getLogger("func-python-logger")


def _vis_to_im(griddata, freq):
    return np.round(griddata.griddata_acc.griddata_wcs.sub([4]).wcs_world2pix(
        np.asarray(freq), 0)[0]).astype(int)


def _lin(wcs, axis, world, dev):
    """Linear world->pixel (origin 0) of one WCS axis on the device."""
    w = wcs.wcs
    return (world - w.crval[axis]) / w.cdelt[axis] + w.crpix[axis] - 1.0


def spatial_mapping(griddata, u, v, w, cf=None):
    """Device version of the reference mapping; u, v, w are f64 device tensors."""
    dev = u.device
    grid_wcs = griddata.griddata_acc.griddata_wcs
    pu_grid = torch.round(_lin(grid_wcs, 0, u, dev)).to(torch.int64)
    pv_grid = torch.round(_lin(grid_wcs, 1, v, dev)).to(torch.int64)
    if cf is None:
        pu_c = torch.round(_lin(grid_wcs, 0, -u, dev)).to(torch.int64)
        pv_c = torch.round(_lin(grid_wcs, 1, -v, dev)).to(torch.int64)
        return pu_grid, pv_grid, pu_c, pv_c
    assert cf.convolutionfunction_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    nw, ndv, ndu = cf.convolutionfunction_acc.shape[2:5]
    cf_wcs = cf.convolutionfunction_acc.cf_wcs
    np.testing.assert_almost_equal(grid_wcs.wcs.cdelt[0], cf_wcs.wcs.cdelt[0], 7)
    np.testing.assert_almost_equal(grid_wcs.wcs.cdelt[1], cf_wcs.wcs.cdelt[1], 7)
    shape = cf["pixels"].data.shape
    if ndu > 1 and ndv > 1:
        gw = grid_wcs.wcs
        wu_grid = gw.crval[0] + gw.cdelt[0] * (pu_grid.to(torch.float64) + 1.0 - gw.crpix[0])
        wv_grid = gw.crval[1] + gw.cdelt[1] * (pv_grid.to(torch.float64) + 1.0 - gw.crpix[1])
        pu_offset = torch.round(_lin(cf_wcs, 2, u - wu_grid, dev)).to(torch.int64)
        pv_offset = torch.round(_lin(cf_wcs, 3, v - wv_grid, dev)).to(torch.int64)
        assert int(pu_offset.min()) >= 0, \
            f"image sampling wrong: DU axis underflows: {int(pu_offset.min())}"
        assert int(pu_offset.max()) < shape[3], f"DU axis overflows: {int(pu_offset.max())}"
        assert int(pv_offset.min()) >= 0, \
            f"image sampling wrong: DV axis underflows: {int(pv_offset.min())}"
        assert int(pv_offset.max()) < shape[4], f"DV axis overflows: {int(pv_offset.max())}"
    else:
        pu_offset = torch.zeros_like(pu_grid)
        pv_offset = torch.zeros_like(pv_grid)
    if nw > 1:
        pwc_pixel = _lin(cf_wcs, 4, w, dev)
        pwc_grid = torch.round(pwc_pixel).to(torch.int64)
        assert int(pwc_grid.min()) >= 0, f"W axis underflows: {int(pwc_grid.min())}"
        assert int(pwc_grid.max()) < shape[2], f"W axis overflows: {int(pwc_grid.max())}"
        pwc_fraction = pwc_pixel - pwc_grid
    else:
        pwc_fraction = torch.zeros_like(pu_grid, dtype=torch.float64)
        pwc_grid = torch.zeros_like(pu_grid)
    return pu_grid, pu_offset, pv_grid, pv_offset, pwc_grid, pwc_fraction


def convolution_mapping_visibility(vis, griddata, chan, cf=None):
    assert vis.visibility_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    dev = _device.device()
    uvw = _device.to_dev(vis.uvw.data, torch.float64, dev).reshape(-1, 3)
    f = float(np.asarray(vis.frequency.data)[chan]) / 299792458.0
    u, v, w = (torch.nan_to_num(uvw[:, k] * f) for k in range(3))
    return spatial_mapping(griddata, u, v, w, cf)


def _maps(vis, griddata, cf, dev):
    nchan = vis.vis.shape[2]
    out = {k: [] for k in ("pu", "pv", "pwc", "pdu", "pdv")}
    for ch in range(nchan):
        pu, pdu, pv, pdv, pwc, _ = convolution_mapping_visibility(vis, griddata, ch, cf)
        for k, a in zip(("pu", "pdu", "pv", "pdv", "pwc"), (pu, pdu, pv, pdv, pwc)):
            out[k].append(a.to(torch.int32))
    return {k: torch.stack(v).contiguous() for k, v in out.items()}


def grid_visibility_to_griddata(vis, griddata, cf):
    assert vis.visibility_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    dev = _device.device()
    nrows, nbaselines, nvchan, nvpol = vis.vis.shape
    nichan, nipol = griddata["pixels"].data.shape[:2]
    vis_to_im = torch.as_tensor(_vis_to_im(griddata, vis.frequency.data), dtype=torch.int32,
                                device=dev)
    fv = torch.nan_to_num(_device.to_dev(vis.visibility_acc.flagged_vis, torch.complex128, dev))
    fw = torch.nan_to_num(_device.to_dev(vis.visibility_acc.flagged_imaging_weight,
                                         torch.float64, dev))
    fv = fv.reshape(nrows * nbaselines, nvchan, nvpol).contiguous()
    fw = fw.reshape(nrows * nbaselines, nvchan, nvpol).contiguous()
    cfp = torch.nan_to_num(_device.to_dev(cf["pixels"].data, torch.complex128, dev)).contiguous()
    grid = torch.zeros(tuple(griddata["pixels"].data.shape), dtype=torch.complex128, device=dev)
    sumwt = torch.zeros((nichan, nipol), dtype=torch.float64, device=dev)
    maps = _maps(vis, griddata, cf, dev)
    skipped = int(kernels.grid_cf(maps, vis_to_im, fv, fw, cfp, grid, sumwt).item())
    if skipped > 0:
        log.warning("warning visibility_to_griddata gridding: skipped %d visbility", skipped)
    griddata["pixels"].data = _device.like_input(torch.nan_to_num(grid), griddata["pixels"].data)
    return griddata, np.nan_to_num(sumwt.cpu().numpy())


def degrid_visibility_from_griddata(vis, griddata, cf):
    assert vis.visibility_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    assert cf.convolutionfunction_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    dev = _device.device()
    newvis = vis.copy(deep=True, zero=True)
    nrows, nbaselines, nvchan, nvpol = vis.vis.shape
    vis_to_im = torch.as_tensor(_vis_to_im(griddata, vis.frequency.data), dtype=torch.int32,
                                device=dev)
    gd = _device.to_dev(griddata["pixels"].data, torch.complex128, dev).contiguous()
    cfp = _device.to_dev(cf["pixels"].data, torch.complex128, dev).contiguous()
    out = torch.zeros((nrows * nbaselines, nvchan, nvpol), dtype=torch.complex128, device=dev)
    maps = _maps(vis, griddata, cf, dev)
    skipped = int(kernels.degrid_cf(maps, vis_to_im, gd, cfp, nrows * nbaselines, nvchan, out).item())
    if skipped > 0:
        log.warning("warning gridding: skipped %d visbility", skipped)
    newvis["vis"].data = _device.like_input(out.reshape(nrows, nbaselines, nvchan, nvpol),
                                           vis["vis"].data)
    return newvis


def _uv_wcs(griddata):
    w = griddata.griddata_acc.griddata_wcs.wcs
    return ((w.crval[0], w.cdelt[0], w.crpix[0]), (w.crval[1], w.cdelt[1], w.crpix[1]))


def _weight_inputs(vis, dev):
    """Device views of uvw [nrow, 3], frequency, weight / flags [nrow, nchan, npol]."""
    nrows, nbaselines, nvchan, nvpol = vis.vis.shape
    nrow = nrows * nbaselines
    uvw = _device.to_dev(vis.uvw.data, torch.float64, dev).reshape(nrow, 3).contiguous()
    freq = _device.to_dev(np.asarray(vis.frequency.data, dtype=float), torch.float64, dev)
    wt = _device.to_dev(vis.weight.data, torch.float64, dev).reshape(nrow, nvchan, nvpol).contiguous()
    fl = _device.to_dev(vis.flags.data, None, dev)
    if fl.dtype not in kernels.FLAG_BYTES:
        fl = fl.to(torch.int64)
    fl = fl.reshape(nrow, nvchan, nvpol).contiguous()
    return uvw, freq, wt, fl


def grid_weights_device(vis, griddata):
    """Weight grid (real f64, device) and sumwt (device) of
    grid_visibility_weight_to_griddata, without leaving the device."""
    assert vis.visibility_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    dev = _device.device()
    nchan, npol, ny, nx = griddata["pixels"].data.shape
    uvw, freq, wt, fl = _weight_inputs(vis, dev)
    v2i = torch.as_tensor(_vis_to_im(griddata, vis.frequency.data), dtype=torch.int32, device=dev)
    grid = torch.zeros((nchan, npol, ny, nx), dtype=torch.float64, device=dev)
    sumwt = torch.zeros((nchan, npol), dtype=torch.float64, device=dev)
    skipped = int(kernels.grid_weights(uvw, freq, wt, fl, v2i, _uv_wcs(griddata), grid, sumwt).item())
    if skipped > 0:
        log.warning("warning visibility_weight_to_griddata gridding: skipped %d visbility", skipped)
    return grid, sumwt


def grid_visibility_weight_to_griddata(vis, griddata):
    """Reference gridding.py:258-334: both the sample's cell and its
    conjugate's receive the flagged weight; returns (griddata, sumwt)."""
    grid, sumwt = grid_weights_device(vis, griddata)
    griddata["pixels"].data = _device.like_input(grid.to(torch.complex128),
                                                 griddata["pixels"].data)
    return griddata, sumwt.cpu().numpy()


def griddata_merge_weights(gd_list):
    """Reference gridding.py:337-359: sum the weight grids onto the centre one."""
    centre = len(gd_list) // 2
    gd = copy.deepcopy(gd_list[centre][0])
    sumwt = gd_list[centre][1]
    frequency = 0.0
    bandwidth = 0.0
    for i, g in enumerate(gd_list):
        if i != centre:
            gd["pixels"].data += g[0]["pixels"].data
            sumwt += g[1]
        frequency += g[0].griddata_acc.griddata_wcs.wcs.crval[3]
        bandwidth += g[0].griddata_acc.griddata_wcs.wcs.cdelt[3]
    gd.griddata_acc.griddata_wcs.wcs.cdelt[3] = bandwidth
    gd.griddata_acc.griddata_wcs.wcs.crval[3] = frequency / len(gd_list)
    return gd, sumwt


def _store(vis, name, value):
    """Write a device result into vis[name] in place, on the variable's side."""
    cur = vis[name].data
    if _device.is_device(cur):
        if cur.dtype == value.dtype and cur.is_contiguous() and cur.data_ptr() == value.data_ptr():
            return
        cur.copy_(value.reshape(cur.shape))
    else:
        cur[...] = value.reshape(cur.shape).cpu().numpy()


def _reweight_device(vis, grid, wcs, v2i, weighting, robustness, sumwt):
    dev = _device.device()
    nrows, nbaselines, nvchan, nvpol = vis.vis.shape
    uvw, freq, wt, fl = _weight_inputs(vis, dev)
    iw = _device.to_dev(vis.imaging_weight.data, torch.float64, dev).reshape(
        nrows * nbaselines, nvchan, nvpol)
    if not iw.is_contiguous():
        iw = iw.contiguous()
    sw = None if sumwt is None else _device.to_dev(np.asarray(sumwt, dtype=float) if not
                                                   _device.is_device(sumwt) else sumwt,
                                                   torch.float64, dev).contiguous()
    kernels.reweight(uvw, freq, wt, fl, v2i, wcs, grid, iw, weighting=weighting,
                     robustness=robustness, sumwt=sw)
    _store(vis, "imaging_weight", iw)
    return vis


def griddata_visibility_reweight(vis, griddata, weighting="uniform", robustness=0.0, sumwt=None):
    """Reference gridding.py:362-499: natural copies the weight; uniform
    divides the flagged weight by the gridded weight at the sample's cell;
    robust (Briggs) divides by 1 + f2 * gridded weight; samples off the grid
    or on an empty cell get zero."""
    if griddata is not None:
        assert vis.visibility_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    assert weighting in ["natural", "uniform", "robust"], f"Weighting {weighting} not supported"
    if weighting == "natural":
        return _reweight_device(vis, None, None, None, "natural", robustness, None)
    dev = _device.device()
    grid = torch.real(_device.to_dev(griddata["pixels"].data, None, dev)).to(torch.float64)
    v2i = torch.as_tensor(_vis_to_im(griddata, vis.frequency.data), dtype=torch.int32, device=dev)
    return _reweight_device(vis, grid.contiguous(), _uv_wcs(griddata), v2i, weighting, robustness,
                            sumwt)


def _centred(x, inverse):
    x = torch.fft.ifftshift(x, dim=(-2, -1))
    x = torch.fft.ifft2(x) if inverse else torch.fft.fft2(x)
    return torch.fft.fftshift(x, dim=(-2, -1))


def fft_griddata_to_image(griddata, template, gcf=None):
    dev = _device.device()
    g = _device.to_dev(griddata["pixels"].data, torch.complex128, dev)
    ny, nx = g.shape[-2], g.shape[-1]
    im = _centred(g, True) * float(nx) * float(ny)
    if gcf is not None:
        im = im * _device.to_dev(gcf["pixels"].data, None, dev)
    return Image.constructor(data=_device.like_input(im, griddata["pixels"].data),
                             polarisation_frame=griddata.griddata_acc.polarisation_frame,
                             wcs=template.image_acc.wcs)


def fft_image_to_griddata(im, griddata, gcf=None):
    assert im.image_acc.polarisation_frame == griddata.griddata_acc.polarisation_frame
    dev = _device.device()
    x = _device.to_dev(im["pixels"].data, torch.complex128, dev)
    if gcf is not None:
        x = x * _device.to_dev(gcf["pixels"].data, None, dev)
    griddata["pixels"].data = _device.like_input(_centred(x, False), griddata["pixels"].data)
    return griddata
