"""Host side of create_awterm_convolutionfunction: the recipe composed from
the package's numpy fourier_transforms (tests/wkernel_restatement.py) against
the same recipe run with the reference's functions (tests/golden/wkernel_*.npz,
bit for bit), the cf_wcs, shapes and grid correction, and every refusal --
none of which touches a device."""

import numpy as np
import pytest

import wkernel_restatement as W
from conftest import golden


def _restated(case):
    c = W.CASES[case]
    cf = W.restate_awterm(W.case_image(case), c["nw"], c["wstep"], c["os"], c["support"],
                          c["use_aaf"], c["N"], W.case_pb(case), normalise=False)
    return cf[:, :, list(c["planes"])]


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_restatement_equals_reference_recipe(case):
    g = golden(f"wkernel_{case}.npz")
    c = W.CASES[case]
    cf = _restated(case)
    nb = 1 if c["pb"] is None else c["pb"][0] * c["pb"][1]
    nd = 2 * (c["os"] // 2) + 1
    assert g["cf"].shape == (nb, len(c["planes"]), nd, nd, c["support"], c["support"])
    np.testing.assert_array_equal(cf.reshape(g["cf"].shape), g["cf"])


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_fixture_errors_are_what_they_claim(case):
    """S of a fixture is the larger error of its two float64 forms against
    the longdouble one; it grows with |w| (the cancellation in 1 - sqrt(1 -
    r2)) from below 1e-15 at w = 0."""
    g = golden(f"wkernel_{case}.npz")
    ld = golden(f"wkernel_{case}_ld.npz")["cf_ld"]
    direct = golden(f"wkernel_{case}_direct.npz")["cf_direct"]
    s = max(np.abs(g["cf"] - ld).max(), np.abs(direct - ld).max()) / np.abs(ld).max()
    # cf_ld is stored rounded to float64: half an ulp of the peak at the most
    assert abs(s - float(g["S"])) <= 2.3e-16
    wmax = np.abs(g["w"]).max()
    assert float(g["S"]) < (1e-15 if wmax <= 10 else 2e-16 * wmax)


def test_even_oversampling_end_planes_hold_the_same_samples():
    cf = golden("wkernel_a.npz")["cf"][0]
    h2 = 8
    np.testing.assert_array_equal(cf[:, :, h2, :, 1:], cf[:, :, 0, :, :-1])
    np.testing.assert_array_equal(cf[:, h2, :, 1:, :], cf[:, 0, :, :-1, :])


def test_geometry_wcs_and_grid_correction():
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.fourier_transforms.fft_coordinates import coordinates, grdsf
    from ska_sdp_func_python_amd.grid_data import convolution_functions as C
    im = W.case_image("c")                      # 2 channels, linearnp
    g = C.cf_geometry(im, nw=5, wstep=25.0, oversampling=4, support=12)
    assert (g["nchan"], g["npol"], g["nx"], g["N"], g["h"], g["nd"]) == (2, 2, 64, 32, 2, 5)
    assert g["w"] == [-50.0, -25.0, 0.0, 25.0, 50.0]
    assert g["fov"] == 64 * float(np.deg2rad(abs(im.image_acc.wcs.wcs.cdelt[1])))
    assert abs(g["fov"] - 64 * 0.004) < 1e-15
    assert C.cf_geometry(im, polarisation_frame=dm.PolarisationFrame("linear"))["npol"] == 4
    assert C.cf_geometry(im, oversampling=5)["nd"] == 5
    # the default far-field size: the smallest even number >= max(support + 2, 32)
    assert [C.default_farfield_npixel(s) for s in (2, 16, 30, 32, 40)] == [32, 32, 32, 34, 42]

    w = C.cf_wcs_for_image(im, 5, 25.0, 4, 12).wcs
    gw = dm.create_griddata_from_image(im).griddata_acc.griddata_wcs.wcs
    cdu, cdv = gw.cdelt[0], gw.cdelt[1]
    assert cdu < 0 < cdv
    assert w.ctype == ["UU", "VV", "DUU", "DVV", "WW", "STOKES", "FREQ"]
    np.testing.assert_array_equal(w.crpix, [7, 7, 3, 3, 3, 1, 1])
    np.testing.assert_array_equal(w.cdelt, [cdu, cdv, cdu / 4, cdv / 4, 25.0, 1, 2.0e6])
    np.testing.assert_array_equal(w.crval, [0, 0, 0, 0, 0, 1, 1.0e8])

    gcf = C.grid_correction_pixels(2, 2, 64, use_aaf=True)
    tg = grdsf(np.abs(2 * coordinates(64)))[0]
    assert gcf.shape == (2, 2, 64, 64) and gcf.dtype == np.float64
    np.testing.assert_array_equal(gcf, np.broadcast_to(1 / np.outer(tg, tg), gcf.shape))
    np.testing.assert_array_equal(gcf[0, 0], golden("wkernel_e2e.npz")["gcf"][0, 0])
    np.testing.assert_array_equal(C.grid_correction_pixels(1, 4, 8, use_aaf=False),
                                  np.ones((1, 4, 8, 8)))


def _refuses(im, **kw):
    from ska_sdp_func_python_amd.grid_data import create_awterm_convolutionfunction
    with pytest.raises(ValueError):
        create_awterm_convolutionfunction(im, **kw)


def test_refusals_come_before_any_device_work():
    """Every refusal is a ValueError raised on the host: this test runs
    without a device, where anything later would raise HipLibraryError."""
    import math
    from ska_sdp_func_python_amd import datamodels as dm
    im = W.case_image("a")
    nonsquare = im.copy(deep=True)
    nonsquare["pixels"].data = np.zeros((1, 1, 64, 48))
    _refuses(nonsquare)
    cells = im.copy(deep=True)
    cells.attrs["wcs"] = cells.image_acc.wcs.deepcopy()
    cells.image_acc.wcs.wcs.cdelt[1] = math.degrees(0.005)
    _refuses(cells)
    _refuses(im, support=15)
    _refuses(im, support=0)
    _refuses(im, support=16, farfield_npixel=33)
    _refuses(im, support=16, farfield_npixel=16)
    _refuses(im, oversampling=0)
    _refuses(im, nw=0)
    _refuses(im, farfield_npixel=32, pb=np.ones((1, 1, 32, 30)))
    _refuses(im, farfield_npixel=32, pb=np.ones((1, 2, 32, 32)))
    _refuses(im, farfield_npixel=32, pb=np.ones((1, 1, 32, 32)),
             polarisation_frame=dm.PolarisationFrame("linear"))
    from ska_sdp_func_python_amd.grid_data import create_pswf_convolutionfunction
    with pytest.raises(ValueError):
        create_pswf_convolutionfunction(im, support=5)
