"""Every accumulation strategy of the imaging-weight gridder
(csrc/weighting.hip) against oracle/weighting_oracle.py, on the cases of
tests/weighting_cases.py: rectangular grids, off-centre and fractional
reference pixels, the LDS window on and off and clipped to the grid, the
conjugate-mirror fold with its rounding-tie branch, 256- and 1024-thread
blocks, sumwt and freq / c in LDS or in global memory.  Weights are dyadic, so
grid, sumwt, skip count and uniform weights are compared bit for bit;
tests/test_weighting_cases_cpu.py shows that each case takes the branch it is
named for."""

import functools
import math

import numpy as np
import pytest
import torch

import weighting_cases as wc
import weighting_oracle as wo

pytestmark = pytest.mark.gpu
RTOL = 1e-12

VARIANTS = {
    "nomirror": {"SDP_HIP_WEIGHT_NOMIRROR": "1"},
    "win0": {"SDP_HIP_WEIGHT_WIN": "0"},
    "win8": {"SDP_HIP_WEIGHT_WIN": "8"},
    "nt256": {"SDP_HIP_WEIGHT_NT": "256"},
    "nomirror_win0": {"SDP_HIP_WEIGHT_NOMIRROR": "1", "SDP_HIP_WEIGHT_WIN": "0"},
}
VARIANT_CASES = ["rect_mirror", "rect_offcentre", "rect_edge", "ties", "ties_rect"]


def _dev(x, dtype=None):
    return None if x is None else torch.as_tensor(np.array(x), device="cuda", dtype=dtype)


@functools.lru_cache(maxsize=None)
def _ref_reweight(name, mode, robustness=0.0, with_sumwt=False):
    """The oracle's imaging weights of a case, computed once."""
    c = wc.case(name)
    out = wo.reweight(c["uvw"], c["freq"], c["fwt"], c["fimw"], c["v2i"], c["wcs"], c["ref_grid"],
                      mode, robustness=robustness, sumwt=c["ref_sumwt"] if with_sumwt else None)
    out.setflags(write=False)
    return out


def _operands(c, wt=None):
    return (_dev(c["uvw"]), _dev(c["freq"]), _dev(c["wt"] if wt is None else wt),
            _dev(c["flags"]), _dev(c["v2i"], torch.int32))


def _grid(c, wt=None):
    from ska_sdp_func_python_amd import kernels
    ops = _operands(c, wt)
    grid = torch.zeros((c["g_nchan"], c["npol"], c["ny"], c["nx"]), dtype=torch.float64,
                       device="cuda")
    sumwt = torch.zeros((c["g_nchan"], c["npol"]), dtype=torch.float64, device="cuda")
    skipped = kernels.grid_weights(*ops, c["wcs"], grid, sumwt)
    return ops, grid, sumwt, int(skipped.item())


def _reweight(c, ops, grid, mode, **kw):
    from ska_sdp_func_python_amd import kernels
    iw = _dev(c["imw"])
    kernels.reweight(*ops, c["wcs"], grid, iw, mode, **kw)
    return iw.cpu().numpy()


def _check_against_oracle(c):
    ops, grid, sumwt, skipped = _grid(c)
    assert skipped == c["ref_skip"] > 0
    got = grid.cpu().numpy()
    bad = np.argwhere(got != c["ref_grid"])
    assert bad.size == 0, f"{len(bad)} cells differ, first (chan, pol, y, x) {bad[:4].tolist()}"
    assert np.array_equal(sumwt.cpu().numpy(), c["ref_sumwt"]), (sumwt.cpu().numpy(),
                                                                  c["ref_sumwt"])
    assert np.array_equal(_reweight(c, ops, grid, "uniform"), _ref_reweight(c["name"], "uniform"))
    assert np.array_equal(_reweight(c, ops, grid, "natural"), c["wt"])
    for rob, sw in ((0.0, None), (-0.7, c["ref_sumwt"])):
        ref = _ref_reweight(c["name"], "robust", rob, sw is not None)
        got = _reweight(c, ops, grid, "robust", robustness=rob, sumwt=_dev(sw))
        np.testing.assert_allclose(got, ref, rtol=RTOL, err_msg=f"robust {rob}")


@pytest.mark.parametrize("name", sorted(wc.GEOMETRY))
def test_geometry_matches_oracle(name):
    """Grid, sumwt, skip count and uniform weights exact, robust weights to
    RTOL (the order of the f2 reduction), natural weights a copy."""
    _check_against_oracle(wc.case(name))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", VARIANT_CASES)
def test_strategy_variant_matches_oracle(name, variant, monkeypatch):
    """The same cases with the mirror fold off, the window off or 8 cells
    wide, and 256-thread blocks: each against the oracle, bit for bit."""
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    _check_against_oracle(wc.case(name))


@pytest.mark.parametrize("name", wc.TIE_CASES)
def test_tie_samples_alone(name):
    """Only the rounding-tie samples carry weight, so everything on the grid
    comes from the tie branch: each plane holds 2 * sum(w[tie]), sumwt the
    same, and the cells are the oracle's."""
    c = wc.case(name)
    wt = c["wt"] * c["tie"][:, :, None]
    fwt = c["fwt"] * c["tie"][:, :, None]
    expect = np.zeros((c["g_nchan"], c["npol"]))
    for ch in range(c["nchan"]):
        expect[c["v2i"][ch]] += 2.0 * fwt[:, ch, :].sum(0)
    assert (expect > 0).all()
    _, grid, sumwt, skipped = _grid(c, wt)
    assert skipped == c["ref_skip"]
    got = grid.cpu().numpy()
    assert np.array_equal(got.sum((2, 3)), expect), (got.sum((2, 3)), expect)
    assert np.array_equal(sumwt.cpu().numpy(), expect), (sumwt.cpu().numpy(), expect)
    ref_grid, ref_sumwt, _ = wo.grid_weights(c["uvw"], c["freq"], fwt, c["v2i"], c["wcs"],
                                             c["g_nchan"], c["ny"], c["nx"])
    assert np.array_equal(ref_sumwt, expect)
    assert np.array_equal(got, ref_grid)


def test_reweight_nan_grid_cell_keeps_flagged_imaging_weight():
    """A NaN grid weight is neither > 0 nor <= 0: the reference leaves the
    flagged imaging weight of those samples alone.  Rectangular grid."""
    c = wc.case("rect_mirror")
    ops, grid, _, _ = _grid(c)
    pu, pv, _, _, ok = wc.cells(c)
    # the cell (of image channel 0, pol 1) that holds the most samples
    flat = (pv * c["nx"] + pu)[ok & (c["v2i"][None, :] == 0)]
    y, x = divmod(int(np.bincount(flat).argmax()), c["nx"])
    ref_grid = c["ref_grid"].copy()
    assert ref_grid[0, 1, y, x] > 0
    ref_grid[0, 1, y, x] = np.nan
    grid[0, 1, y, x] = float("nan")
    got = _reweight(c, ops, grid, "uniform")
    ref = wo.reweight(c["uvw"], c["freq"], c["fwt"], c["fimw"], c["v2i"], c["wcs"], ref_grid,
                      "uniform")
    hit = ok & (pv == y) & (pu == x) & (c["v2i"][None, :] == 0)
    assert hit.sum() >= 2 and (c["fimw"][hit, 1] > 0).any()
    assert np.array_equal(got[hit, 1], c["fimw"][hit, 1])
    assert not np.isnan(got).any() and np.array_equal(got, ref)


@pytest.mark.parametrize("name", ["frac_crpix", "rect_mirror"])
def test_tapers_on_odd_shapes(name):
    """Gaussian and Tukey tapers on 9 channels x 1 pol without flags and 12
    channels x 4 pols with int32 flags."""
    from ska_sdp_func_python_amd import kernels
    c = wc.case(name)
    if name == "frac_crpix":
        freq, imw, flags = c["freq"], c["imw"], None
        assert imw.shape[1:] == (9, 1) and c["flags"] is None
    else:
        freq, imw = c["freq"][:12], c["imw"][:, :12]
        flags = c["flags"][:, :12].astype(np.int32)
        assert imw.shape[1:] == (12, 4)
    fimw = imw if flags is None else imw * (1 - flags)
    beam = 0.5 * wo.C_M_S / (freq.max() * np.abs(c["uvw"][:, :2]).max())
    for kind, param, ref in (
            ("gaussian", math.pi ** 2 * beam ** 2 / (4 * math.log(2)),
             wo.taper_gaussian(c["uvw"], freq, fimw, beam)),
            ("tukey", 0.25, wo.taper_tukey(c["uvw"], freq, fimw, 0.25))):
        d_iw = _dev(imw)
        kernels.taper(_dev(c["uvw"]), _dev(freq), _dev(flags), d_iw, kind, param)
        # 0.5 (1 + cos) cancels near the taper's zero: absolute 1e-15 there
        np.testing.assert_allclose(d_iw.cpu().numpy(), ref, rtol=1e-13, atol=1e-15, err_msg=kind)


def test_wrappers_on_a_rectangular_griddata():
    """grid_visibility_weight_to_griddata / griddata_visibility_reweight with
    device tensors on a 96 x 160 GridData whose WCS is built by hand: ny and
    nx reach the C ABI in the right order."""
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.grid_data import (grid_visibility_weight_to_griddata,
                                                   griddata_visibility_reweight)
    from ska_sdp_func_python_amd.grid_data.gridding import _vis_to_im
    c = wc.case("rect_mirror")
    pf = dm.PolarisationFrame("linear")
    nrow, nchan, npol = c["wt"].shape
    shape = (1, nrow, nchan, npol)
    (uval, udel, upix), (vval, vdel, vpix) = c["wcs"]
    f = c["freq"].copy()
    per = nchan // c["g_nchan"]
    gw = dm.WCS(4, ["UU", "VV", "STOKES", "FREQ"], [upix, vpix, 1.0, 1.0],
                [udel, vdel, 1.0, per * (f[1] - f[0])], [uval, vval, 1.0, f[:per].mean()])
    gd = dm.GridData.constructor(np.zeros((c["g_nchan"], npol, c["ny"], c["nx"]), complex), gw, pf)
    assert np.array_equal(_vis_to_im(gd, f), c["v2i"])

    def vis():
        arrs = dict(uvw=c["uvw"].reshape(1, nrow, 3), weight=c["wt"].reshape(shape),
                    flags=c["flags"].reshape(shape), imaging_weight=c["imw"].reshape(shape),
                    vis=np.zeros(shape, complex))
        arrs = {k: _dev(v) for k, v in arrs.items()}
        return dm.Visibility.constructor(
            frequency=f, channel_bandwidth=np.full(nchan, f[1] - f[0]),
            phasecentre=dm.SkyCoord(0, -0.5), time=np.zeros(1),
            baselines=np.stack(np.triu_indices(111, 1), 1)[:nrow], polarisation_frame=pf, **arrs)

    gd, sumwt = grid_visibility_weight_to_griddata(vis(), gd)
    pixels = gd["pixels"].data
    pixels = pixels.cpu().numpy() if isinstance(pixels, torch.Tensor) else np.asarray(pixels)
    assert pixels.shape == c["ref_grid"].shape
    assert np.array_equal(pixels.real, c["ref_grid"]) and not pixels.imag.any()
    assert np.array_equal(sumwt, c["ref_sumwt"])
    v = griddata_visibility_reweight(vis(), gd, weighting="uniform")
    ref = _ref_reweight("rect_mirror", "uniform")
    assert np.array_equal(v.imaging_weight.data.cpu().numpy().reshape(ref.shape), ref)
