"""The numpy paths of imaging/imaging_helpers.py, the host functions added to
imaging/base.py and the argument checks of imaging/wg.py against what the
reference's own functions returned (tests/golden/imghelp_*.npz, written by
tests/golden/make_golden_imghelp.py from the inputs of tests/imghelp_case.py).
Every comparison is for equality, the signs of zeros included."""

import numpy as np
import pytest

from conftest import golden
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd import imaging
from ska_sdp_func_python_amd.imaging import base, imaging_helpers as ih, wg

import imghelp_case as C


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- sum_invert_results, remove_sumwt ------------------------------------------
@pytest.mark.parametrize("name", list(C.INVERT_CASES))
def test_sum_invert_results_matches_reference(name):
    g = golden("imghelp_sum.npz")
    image_list = C.invert_list(name)
    before = C.invert_case(name)
    im, sumwt = ih.sum_invert_results(image_list)
    assert same_bits(im["pixels"].data, g[f"invert_{name}_pixels"])
    assert same_bits(sumwt, g[f"invert_{name}_sumwt"])
    first = image_list[0][0]
    assert im.attrs["clean_beam"] == C.CLEAN_BEAM
    assert im.image_acc.polarisation_frame == first.image_acc.polarisation_frame
    assert np.array_equal(im.image_acc.wcs.wcs.crval, first.image_acc.wcs.wcs.crval)
    for entry, b in zip(image_list, before):  # the inputs are left alone
        assert entry is None or (same_bits(entry[0]["pixels"].data, b[0])
                                 and same_bits(entry[1], b[1]))


def test_sum_invert_results_of_one_copies_the_image_and_keeps_sumwt():
    image_list = C.invert_list("one")
    im, sumwt = ih.sum_invert_results(image_list)
    assert sumwt is image_list[0][1]
    assert im is not image_list[0][0]
    assert not np.shares_memory(im["pixels"].data, image_list[0][0]["pixels"].data)
    assert same_bits(im["pixels"].data, image_list[0][0]["pixels"].data)  # not normalised


def test_sum_invert_results_zeroes_a_plane_without_weight():
    im, sumwt = ih.sum_invert_results(C.invert_list("zero_plane"))
    plane = im["pixels"].data[C.INVERT_CASES["zero_plane"]["zero_plane"]]
    assert sumwt[C.INVERT_CASES["zero_plane"]["zero_plane"]] == 0.0
    assert not plane.any() and not np.signbit(plane).any()
    assert np.isfinite(im["pixels"].data).all()


def test_remove_sumwt():
    pairs = C.invert_list("negative")
    images = ih.remove_sumwt(pairs)
    assert len(images) == len(pairs) and all(a is b[0] for a, b in zip(images, pairs))


# ---- sum_predict_results ---------------------------------------------------------
def test_sum_predict_results_matches_reference_and_sums_in_place():
    results = C.predict_list()
    first_data = results[1]["vis"].data
    others = [None if r is None else r["vis"].data.copy() for r in results]
    summed = ih.sum_predict_results(results)
    assert summed is results[1]
    assert summed["vis"].data is first_data
    assert same_bits(summed["vis"].data, golden("imghelp_sum.npz")["predict_vis"])
    for r, b in zip(results[2:], others[2:]):
        assert r is None or same_bits(r["vis"].data, b)


def test_sum_predict_results_edge_cases():
    assert ih.sum_predict_results([None, None]) is None
    one = C.make_vis("low")
    assert ih.sum_predict_results([None, one]) is one
    with pytest.raises(AssertionError):
        ih.sum_predict_results([C.make_vis("low"), C.make_vis("mid")])


# ---- threshold_list ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.THRESHOLD_CASES))
def test_threshold_list_matches_reference(name):
    images, threshold, fraction, moment0 = C.THRESHOLD_CASES[name]
    got = ih.threshold_list(C.threshold_list_input(images), threshold, fraction,
                            use_moment0=moment0)
    assert same_bits(np.float64(got), golden("imghelp_threshold.npz")[name])


def test_threshold_list_cases_take_the_branches_they_are_named_for():
    g = golden("imghelp_threshold.npz")
    assert g["cubes_moment_abs"] == 10.0 and g["cubes_refchan_abs"] == 4.0
    assert 0.0 < g["cubes_moment_frac"] < 10.0 and 0.0 < g["cubes_refchan_frac"] < 4.0
    assert g["negative_moment"] > 1.0 and g["negative_refchan"] > 1.0
    # the peak of the channel mean is where the middle channel is 0
    assert g["summed_moment"] == np.abs((5.0 + 0.0 + 4.0) / 3) and g["summed_refchan"] == 1.5


def test_threshold_list_refuses_nan_in_moment_mode():
    images = C.threshold_list_input("cubes")
    images[2]["pixels"].data[1, 0, 3, 3] = np.nan
    with pytest.raises(AssertionError, match="NaNs present in image data"):
        ih.threshold_list(images, 0.0, 0.1, use_moment0=True)


# ---- create_image_from_visibility ----------------------------------------------------
@pytest.mark.parametrize("name", list(C.IMAGE_CASES))
def test_create_image_from_visibility_matches_reference(name):
    g = golden("imghelp_image.npz")
    kind, kwargs = C.IMAGE_CASES[name]
    im = base.create_image_from_visibility(C.make_vis(kind), **C.image_kwargs(kwargs))
    for key, value in C.image_summary(im).items():
        assert same_bits(value, g[f"{name}_{key}"]), key
    assert im["pixels"].data.dtype == np.float64 and not im["pixels"].data.any()


def test_create_image_from_visibility_cell_sizes():
    g = golden("imghelp_image.npz")
    critical = g["too_large_cdelt"][1]
    assert g["default_cdelt"][1] == 0.5 * critical  # halving is exact
    assert g["zero_cell_cdelt"][1] == critical
    assert g["no_override_cdelt"][1] == np.degrees(1.0)
    assert g["mfs_shape"][0] == 1 and g["all_channels_shape"][0] == 3 and g["multi_mfs_shape"][0] == 2
    assert g["explicit_crval"][3] == 1.1e9 and g["explicit_cdelt"][3] == 5.0e7
    assert g["polarised_shape"][1] == 4 and str(g["polarised_frame"]) == "stokesIQUV"


def test_create_image_from_visibility_refuses_an_unknown_spectral_mode():
    kind, kwargs = C.IMAGE_REFUSED
    with pytest.raises(ValueError, match="unknown spectral mode"):
        base.create_image_from_visibility(C.make_vis(kind), **kwargs)


# ---- advise_wide_field -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.ADVISE_CASES))
def test_advise_wide_field_matches_reference(name):
    g = golden("imghelp_advise.npz")
    kind, kwargs = C.ADVISE_CASES[name]
    advice = base.advise_wide_field(C.make_vis(kind), **kwargs)
    assert list(advice) == list(g[f"{name}_keys"])
    for key, value in advice.items():
        want = g[f"{name}_{key}"]
        assert np.asarray(value).dtype.kind == want.dtype.kind, key
        assert np.asarray(value) == want, key


def test_advise_wide_field_assertions():
    with pytest.raises(AssertionError, match="all uvw are zero"):
        base.advise_wide_field(C.make_vis("low", uvw=np.zeros((C.NT, C.NB, 3))), verbose=False)
    with pytest.raises(AssertionError, match="greater than zero"):
        base.advise_wide_field(C.make_vis("low", diameter=[38.0, 0.0]), verbose=False)


def test_configuration_diameter_is_optional():
    assert dm.Configuration("MID").name == "MID"
    assert not hasattr(dm.Configuration("MID"), "diameter")
    assert dm.Configuration("MID", diameter=15.0).diameter.data == 15.0
    assert np.array_equal(dm.Configuration("LOW", diameter=[38.0, 35.0]).diameter.data, [38.0, 35.0])


# ---- rad_deg_arcsec, visibility_recentre, wg -------------------------------------------------
def test_rad_deg_arcsec_strings():
    want = golden("imghelp_advise.npz")["rad_deg_arcsec"]
    assert [base.rad_deg_arcsec(x) for x in C.RAD_DEG_ARCSEC_INPUTS] == [str(s) for s in want]


def test_visibility_recentre():
    uvw, dl, dm_ = C.recentre_input()
    before = uvw.copy()
    assert same_bits(base.visibility_recentre(uvw, dl, dm_), golden("imghelp_advise.npz")["recentre"])
    assert same_bits(uvw, before)


def test_wg_functions_refuse_a_model_that_is_not_canonical():
    model = C.make_image(np.zeros((1, 1, 8, 8)), pol_frame="stokesI")
    model.image_acc.wcs.wcs.ctype[3] = "MOMENT"
    vis = C.make_vis("low")
    with pytest.raises(ValueError, match="WG:The image model is not canonical"):
        wg.predict_wg(vis, model)
    with pytest.raises(ValueError, match="WG:The image model is not canonical"):
        wg.invert_wg(vis, model, dopsf=True, normalise=False, threads=2, verbosity=1)


def test_the_imaging_package_exports_the_new_functions():
    for name in ("sum_invert_results", "remove_sumwt", "sum_predict_results", "threshold_list",
                 "create_image_from_visibility", "advise_wide_field", "rad_deg_arcsec",
                 "visibility_recentre", "invert_wg", "predict_wg"):
        assert callable(getattr(imaging, name))
