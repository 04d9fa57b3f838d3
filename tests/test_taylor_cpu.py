"""CPU: the frequency Taylor-term functions of image cubes, image lists and
sky-component lists on numpy pixels against the reference's own results
(tests/golden/taylor_cube.npz, taylor_skycomp.npz; make_golden_taylor.py).

Weights-only results (moments, rebuilt cubes, transposed and gathered
components) are reproduced bit for bit.  Results that go through
``numpy.linalg.pinv`` or ``polyfit`` depend on LAPACK's SVD, whose last bits
may differ between machines: they are compared bit for bit against the
mul-then-add loop taylor_case.mix_loop with the pseudo-inverse computed in
this process, and against the fixture within

    64 * eps * cond_2(coupling) * max|golden|

-- the perturbation bound of a backward-stable pseudo-inverse is O(eps *
cond), and 64 covers the dimension constant of matrices of at most 20
entries.
"""

import numpy as np
import pytest

from conftest import golden
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd import sky_component as sc
from ska_sdp_func_python_amd.image import taylor_terms as tt

import taylor_case as T

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def g():
    return golden("taylor_cube.npz")


@pytest.fixture(scope="module")
def gs():
    return golden("taylor_skycomp.npz")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_within_cond_bound(got, want, cond, what):
    bound = 64 * EPS * cond * np.abs(want).max()
    err = np.abs(np.asarray(got) - want).max()
    assert err <= bound, f"{what}: error {err:.3e} exceeds 64 eps cond max|golden| = {bound:.3e}"


def wcs_fields(wcs):
    w = wcs.wcs
    return (list(w.ctype), list(w.crval), list(w.crpix), list(w.cdelt), list(w.cunit))


def pixels_of(g, tag):
    return g["cube"].astype(np.float32) if tag else g["cube"]


# ---- moments of a cube -----------------------------------------------------------
@pytest.mark.parametrize("tag", ["", "_f32"])
@pytest.mark.parametrize("rtag", ["", "_ref"])
def test_cube_moments_match_the_reference(g, tag, rtag):
    im = T.make_cube(pixels_of(g, tag))
    before = wcs_fields(im.image_acc.wcs)
    rf = float(g["explicit_reference"]) if rtag else None
    moments = tt.calculate_image_frequency_moments(im, reference_frequency=rf, nmoment=3)
    assert same_bits(moments["pixels"].data, g[f"moments3{rtag}{tag}"])
    w = moments.image_acc.wcs.wcs
    assert (w.ctype[3], w.crval[3], w.crpix[3], w.cdelt[3], w.cunit[3]) == ("MOMENT", 0.0, 1.0, 1.0, "")
    assert wcs_fields(moments.image_acc.wcs)[0][:3] == before[0][:3]
    assert wcs_fields(im.image_acc.wcs) == before
    assert moments.image_acc.polarisation_frame == dm.PolarisationFrame(T.POL_FRAME)
    # the restatement that the GPU tests compare against says the same
    wts = T.weights(g["frequency"], g["frequency"][2] if rf is None else rf, 3).T
    assert same_bits(T.mix_loop(wts, list(im["pixels"].data)), moments["pixels"].data)


def test_cube_moments_default_reference_is_the_middle_channel(g):
    im = T.make_cube(g["cube"])
    a = tt.calculate_image_frequency_moments(im, nmoment=2)["pixels"].data
    b = tt.calculate_image_frequency_moments(im, reference_frequency=g["frequency"][2],
                                             nmoment=2)["pixels"].data
    assert same_bits(a, b)
    # moment 0 is the plain channel sum from +0.0: a -0.0 in every channel gives +0.0
    assert not np.signbit(a[0, 0, 5, 6]) and a[0, 0, 5, 6] == 0.0


def test_cube_moments_error_cases(g):
    im = T.make_cube(g["cube"])
    with pytest.raises(AssertionError):
        tt.calculate_image_frequency_moments(g["cube"], nmoment=1)
    bad = T.make_cube(g["cube"])
    bad.image_acc.wcs.wcs.ctype[3] = "MOMENT"
    with pytest.raises(AssertionError):
        tt.calculate_image_frequency_moments(bad, nmoment=1)
    for nmoment in (0, -1):
        with pytest.raises(AssertionError):
            tt.calculate_image_frequency_moments(im, nmoment=nmoment)
    with pytest.raises(AssertionError,
                       match="Number of moments 6 cannot exceed the number of channels 5"):
        tt.calculate_image_frequency_moments(im, nmoment=6)
    assert tt.calculate_image_frequency_moments(im, nmoment=5)["pixels"].shape[0] == 5


def test_cube_moments_report_nans(g):
    pixels = g["cube"].copy()
    pixels[-1, -1, -1, -1] = np.nan
    with pytest.raises(AssertionError, match="NaNs present in image data"):
        tt.calculate_image_frequency_moments(T.make_cube(pixels), nmoment=2)
    # inf in the reference channel meets its weight 0 in moment 1
    pixels = g["cube"].copy()
    pixels[2, 0, 4, 4] = np.inf
    with np.errstate(invalid="ignore"):
        with pytest.raises(AssertionError, match="NaNs present in moment data"):
            tt.calculate_image_frequency_moments(T.make_cube(pixels), nmoment=2)
        assert np.isinf(tt.calculate_image_frequency_moments(
            T.make_cube(pixels), nmoment=1)["pixels"].data[0, 0, 4, 4])


# ---- a cube rebuilt from Taylor terms ----------------------------------------------
@pytest.mark.parametrize("tag", ["", "_f32"])
@pytest.mark.parametrize("rtag", ["", "_ref"])
def test_rebuilt_cube_matches_the_reference(g, tag, rtag):
    im = T.make_cube(pixels_of(g, tag))
    before = wcs_fields(im.image_acc.wcs)
    rf = float(g["explicit_reference"]) if rtag else None
    terms = dm.Image.constructor(g[f"moments3{rtag}{tag}"], dm.PolarisationFrame(T.POL_FRAME),
                                 T.make_wcs())
    rebuilt = tt.calculate_image_from_frequency_taylor_terms(im, terms, reference_frequency=rf)
    assert same_bits(rebuilt["pixels"].data, g[f"rebuilt{rtag}{tag}"])
    assert rebuilt is not im and rebuilt["pixels"].data is not im["pixels"].data
    assert wcs_fields(rebuilt.image_acc.wcs) == before == wcs_fields(im.image_acc.wcs)
    assert rebuilt.image_acc.polarisation_frame == im.image_acc.polarisation_frame
    assert same_bits(im["pixels"].data, pixels_of(g, tag))
    if not tag:
        wts = T.weights(g["frequency"], g["frequency"][2] if rf is None else rf, 3)
        assert same_bits(T.mix_loop(wts, list(terms["pixels"].data)), rebuilt["pixels"].data)


def test_rebuilt_cube_error_cases(g):
    im = T.make_cube(g["cube"])
    pf = dm.PolarisationFrame(T.POL_FRAME)
    none = dm.Image.constructor(np.zeros((0, T.NPOL, T.NY, T.NX)), pf, T.make_wcs())
    with pytest.raises(ValueError, match="the number of taylor terms must be greater than zero"):
        tt.calculate_image_from_frequency_taylor_terms(im, none)
    for shape in ((3, 1, T.NY, T.NX), (3, T.NPOL, T.NY + 1, T.NX), (3, T.NPOL, T.NY, T.NX - 1)):
        with pytest.raises(AssertionError):
            tt.calculate_image_from_frequency_taylor_terms(
                im, dm.Image.constructor(np.zeros(shape), pf, T.make_wcs()))


# ---- decoupled Taylor terms of an image list ----------------------------------------
@pytest.mark.parametrize("tag", ["", "_f32"])
@pytest.mark.parametrize("nmoment", [1, 3])
def test_decoupled_terms_match_the_reference(g, tag, nmoment):
    im_list = T.make_list(pixels_of(g, tag))
    before = [wcs_fields(im.image_acc.wcs) for im in im_list]
    terms = tt.calculate_frequency_taylor_terms_from_image_list(im_list, nmoment=nmoment)
    assert len(terms) == nmoment
    assert all(t["pixels"].data.shape == (1, T.NPOL, T.NY, T.NX) for t in terms)
    got = np.stack([t["pixels"].data for t in terms])
    coupling = T.weights(g["frequency"], g["frequency"][2], nmoment)
    pinv = np.linalg.pinv(coupling, rcond=1e-7)
    loop = T.mix_loop(pinv, [im["pixels"].data for im in im_list])
    assert same_bits(got, loop)
    cond = np.linalg.cond(coupling)
    assert_within_cond_bound(pinv, g[f"pinv{nmoment}"], cond, "pinv")
    assert_within_cond_bound(got, g[f"decoupled{nmoment}{tag}"], cond, "decoupled terms")
    for t in terms:
        w = t.image_acc.wcs.wcs
        assert (w.ctype[3], w.crval[3], w.crpix[3], w.cdelt[3], w.cunit[3]) == \
            ("FREQ", g["frequency"][2], 1.0, 1.0, "Hz")
        assert list(w.ctype[:3]) == before[2][0][:3] and list(w.crval[:3]) == before[2][1][:3]
        assert t.image_acc.polarisation_frame == dm.PolarisationFrame(T.POL_FRAME)
    assert [wcs_fields(im.image_acc.wcs) for im in im_list] == before


def test_decoupled_terms_explicit_reference_and_errors(g):
    im_list = T.make_list(g["cube"])
    rf = float(g["explicit_reference"])
    terms = tt.calculate_frequency_taylor_terms_from_image_list(im_list, nmoment=2,
                                                                reference_frequency=rf)
    assert all(t.image_acc.wcs.wcs.crval[3] == rf for t in terms)
    pinv = np.linalg.pinv(T.weights(g["frequency"], rf, 2), rcond=1e-7)
    assert same_bits(np.stack([t["pixels"].data for t in terms]),
                     T.mix_loop(pinv, [im["pixels"].data for im in im_list]))
    with pytest.raises(ValueError, match="each image must be single channel"):
        tt.calculate_frequency_taylor_terms_from_image_list([T.make_cube(g["cube"])] * 2)


def test_decoupled_terms_recover_an_exact_quadratic(g):
    rng = np.random.default_rng(5)
    coeffs = rng.normal(size=(3, T.NPOL, T.NY, T.NX))
    x = (g["frequency"] - g["frequency"][2]) / g["frequency"][2]
    cube = coeffs[0] + coeffs[1] * x[:, None, None, None] + coeffs[2] * (x ** 2)[:, None, None, None]
    terms = tt.calculate_frequency_taylor_terms_from_image_list(T.make_list(cube), nmoment=3)
    cond = np.linalg.cond(T.weights(g["frequency"], g["frequency"][2], 3))
    assert_within_cond_bound(np.stack([t["pixels"].data[0] for t in terms]), coeffs, cond,
                             "quadratic coefficients")


def test_module_exports():
    assert set(tt.__all__) == {"calculate_image_frequency_moments",
                               "calculate_image_from_frequency_taylor_terms",
                               "calculate_image_list_frequency_moments",
                               "calculate_image_list_from_frequency_taylor_terms",
                               "calculate_frequency_taylor_terms_from_image_list"}
    assert all(callable(getattr(tt, name)) for name in tt.__all__)


# ---- sky components -------------------------------------------------------------------
POL_FRAMES = ["stokesIQUV", "stokesI"]


@pytest.mark.parametrize("pol_frame", POL_FRAMES)
def test_component_taylor_terms_match_the_reference(gs, pol_frame):
    flux = gs[f"flux_{pol_frame}"]
    comps = T.make_components(flux, pol_frame)
    terms = sc.calculate_skycomponent_list_taylor_terms(comps, nmoment=3)
    assert len(terms) == 3 and all(len(per) == 3 for per in terms)
    got = np.array([[t.flux for t in per] for per in terms])
    coupling = T.weights(gs["frequency"], gs["frequency"][2], 3)
    pinv = np.linalg.pinv(coupling, rcond=1e-7)
    npol = flux.shape[2]
    for k in range(3):
        # Stokes I of every channel goes to every polarisation, as in the reference
        loop = T.mix_loop(pinv, [np.full(npol, flux[k, chan, 0]) for chan in range(T.NCHAN)])
        assert same_bits(got[k], loop[:, None, :])
    assert_within_cond_bound(got, gs[f"taylor3_{pol_frame}"], np.linalg.cond(coupling),
                             "component Taylor terms")
    assert all(t.frequency == gs["frequency"][2] and t.name == f"c{k}"
               for k, per in enumerate(terms) for t in per)
    assert same_bits(np.array([c.flux for c in comps]), flux)
    shifted = sc.calculate_skycomponent_list_taylor_terms(comps, nmoment=1,
                                                          reference_frequency=1.03e8)
    assert shifted[0][0].frequency == 1.03e8 and shifted[0][0].flux.shape == (1, npol)


@pytest.mark.parametrize("pol_frame", POL_FRAMES)
def test_component_interpolation_matches_the_reference(gs, pol_frame):
    from numpy.polynomial import polynomial
    flux = gs[f"flux_{pol_frame}"]
    comps = T.make_components(flux, pol_frame)
    interp = sc.interpolate_skycomponents_frequency(comps, nmoment=2)
    got = np.array([c.flux for c in interp])
    assert got.shape == flux.shape
    x = (gs["frequency"] - gs["frequency"][2]) / gs["frequency"][2]
    cond = np.linalg.cond(polynomial.polyvander(x, 1))
    assert_within_cond_bound(got, gs[f"interp2_{pol_frame}"], cond, "interpolated fluxes")
    assert same_bits(np.array([c.flux for c in comps]), flux)
    # as many terms as channels interpolate the fluxes themselves
    full = sc.interpolate_skycomponents_frequency(comps, nmoment=T.NCHAN)
    condn = np.linalg.cond(polynomial.polyvander(x, T.NCHAN - 1))
    assert_within_cond_bound(np.array([c.flux for c in full]), flux, condn, "full-degree fit")


@pytest.mark.parametrize("pol_frame", POL_FRAMES)
def test_component_transpose_and_gather_match_the_reference(gs, pol_frame):
    flux = gs[f"flux_{pol_frame}"]
    comps = T.make_components(flux, pol_frame)
    chans = sc.transpose_skycomponents_to_channels(comps)
    assert len(chans) == T.NCHAN and all(len(per) == 3 for per in chans)
    assert same_bits(np.array([[c.flux for c in per] for per in chans]),
                     gs[f"transposed_{pol_frame}"])
    assert same_bits(np.array([[c.frequency for c in per] for per in chans]),
                     gs[f"transposed_frequency_{pol_frame}"])
    back = sc.gather_skycomponents_from_channels(chans)
    assert same_bits(np.array([c.flux for c in back]), gs[f"gathered_{pol_frame}"])
    assert same_bits(np.array([c.flux for c in back]), flux)
    assert all(same_bits(c.frequency, gs["frequency"]) and c.name == f"c{k}"
               and c.polarisation_frame == dm.PolarisationFrame(pol_frame)
               for k, c in enumerate(back))


def test_component_empty_list():
    assert sc.calculate_skycomponent_list_taylor_terms([], nmoment=3) == [[]]
