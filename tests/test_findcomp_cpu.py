"""find_skycomponents without a GPU: the host restatement
(tests/findcomp_restatement.py) on hand-made cases with the answers written out
by hand, the Python layer of sky_component.operations running on that
restatement in place of the two kernels, and the catalogue helpers against
hand-computed separations.

The restatement is written from numpy and scipy.ndimage.label; it is not a run
of the reference, whose astropy 5.2.2 and photutils 1.8.0 are not available
here: its smoothing and its peaks rest on their documented behaviour (see the
restatement's docstring).
"""

import numpy as np
import pytest
from scipy import ndimage

import findcomp_restatement as fr
import skycomp_restatement as sr
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd.sky_component import operations as ops


# ---- the restatement itself -------------------------------------------------------
def test_labels_sizes_by_hand():
    mask = np.array([[1, 0, 0, 1, 1, 0],
                     [0, 1, 0, 0, 0, 0],
                     [0, 0, 0, 0, 1, 0],
                     [1, 1, 0, 1, 0, 0],
                     [0, 1, 0, 0, 0, 0]], dtype=bool)
    # 8-connected: {(0,0),(1,1)}, {(0,3),(0,4)}, {(2,4),(3,3)}, {(3,0),(3,1),(4,1)}
    want1 = np.array([[1, 0, 0, 2, 2, 0],
                      [0, 1, 0, 0, 0, 0],
                      [0, 0, 0, 0, 3, 0],
                      [4, 4, 0, 3, 0, 0],
                      [0, 4, 0, 0, 0, 0]])
    labels, n = fr.label_mask(mask, 1)
    assert n == 4 and np.array_equal(labels, want1) and labels.dtype == np.int32
    # only the last has three pixels: it becomes segment 1
    labels, n = fr.label_mask(mask, 3)
    assert n == 1 and np.array_equal(labels, np.where(want1 == 4, 1, 0))
    labels, n = fr.label_mask(mask, 4)
    assert n == 0 and not labels.any()


def test_threshold_is_strict_and_mean_in_channel_order():
    planes = np.zeros((2, 3, 4))
    planes[0, 1, 1:3] = 3.0
    planes[1, 1, 1:3] = 1.0  # mean 2.0
    assert fr.segment(planes, 2.0, 1)[1] == 0
    labels, n = fr.segment(planes, np.nextafter(2.0, 0.0), 1)
    assert n == 1 and np.array_equal(np.argwhere(labels == 1), [[1, 1], [1, 2]])
    # float32 planes are summed and divided in float32
    p32 = np.array([1.0, 1e-8, -1.0], dtype=np.float32).reshape(3, 1, 1)
    assert fr.mean_plane(p32).dtype == np.float32 and fr.mean_plane(p32)[0, 0] == 0.0
    assert fr.mean_plane(p32.astype(np.float64))[0, 0] > 0.0


def test_peaks_and_ties_by_hand():
    labels = np.array([[1, 1, 0, 2],
                       [1, 0, 0, 2]], dtype=np.int32)
    planes = np.array([[[5.0, 7.0, 99.0, -3.0],
                        [7.0, 99.0, 99.0, -2.0]],
                       [[-0.0, -1.0, 9.0, 4.0],
                        [0.0, 9.0, 9.0, 4.0]]])
    values, indices = fr.peaks(planes, labels, 2)
    # channel 0: segment 1 has 7 at flat 1 and 4 (first wins); segment 2 is negative
    # channel 1: segment 1 has -0.0 at 0 and 0.0 at 4 (equal: first wins); segment 2 ties
    assert np.array_equal(values, [[7.0, -2.0], [0.0, 4.0]])
    assert np.array_equal(indices, [[1, 7], [0, 3]])


@pytest.mark.parametrize("seed", range(20))
def test_numbering_is_scipys(seed):
    mask = fr.random_mask(45, 70, 0.4, seed)
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
    labels, k = fr.label_mask(mask, 1)
    assert k == n and np.array_equal(labels, lab)
    # and scipy numbers by the first pixel in raster order
    first = [np.flatnonzero(lab.ravel() == s)[0] for s in range(1, n + 1)]
    assert first == sorted(first)


def test_builders():
    ny, nx = fr.SHAPES[0]
    count = {name: fr.label_mask(m, 1)[1] for name, m in fr.mask_cases(ny, nx)}
    for name in ("spiral", "staircase", "staircase_anti", "checkerboard", "full", "comb_down",
                 "comb_up", "comb_right", "comb_left"):
        assert count[name] == 1, name
    assert count["two_spirals"] == 2
    assert count["nested_u"] > 30
    # 4-connectivity would split the staircases into single pixels
    assert ndimage.label(fr.staircase(ny, nx))[1] == min(ny, nx)
    mask, kept = fr.bars(ny, nx, 5)
    assert fr.label_mask(mask, 5)[1] == kept and fr.label_mask(mask, 1)[1] == 2 * kept - 1
    assert fr.label_mask(mask, 4)[1] == 2 * kept - 1


@pytest.mark.parametrize("fwhm, size", [(1, 1), (2, 3), (3, 5), (4, 7), (5, 7)])
def test_kernel_sizes(fwhm, size):
    assert fr.kernel_size(fwhm) == size
    for k in (fr.kernel_of(fwhm), ops.segment_kernel(fwhm)):
        assert k.shape == (size, size)
        assert abs(k.sum() - 1.0) < 1e-15
        assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1])
    assert np.array_equal(fr.kernel_of(fwhm), ops.segment_kernel(fwhm))


def test_kernel_values_and_limit():
    k = fr.kernel_of(2.0)
    sigma = 2.0 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    e, c = np.exp(-1.0 / (2 * sigma ** 2)), np.exp(-2.0 / (2 * sigma ** 2))
    total = 1.0 + 4 * e + 4 * c
    np.testing.assert_allclose(k, np.array([[c, e, c], [e, 1.0, e], [c, e, c]]) / total, rtol=1e-15)
    assert ops.segment_kernel(10.0).shape == (15, 15)
    with pytest.raises(ValueError, match="at most 15"):
        ops.segment_kernel(11.0)


def test_smoothing_by_hand():
    mean = np.zeros((4, 5))
    mean[0, 0] = 2.0
    mean[2, 3] = 1.0
    k = fr.kernel_of(2.0)
    s = fr.smooth(mean, k)
    # a unit pixel spreads the kernel; the corner pixel loses what falls off the image
    np.testing.assert_allclose(s[1:4, 2:5], k, rtol=1e-15)
    np.testing.assert_allclose(s[0:2, 0:2], 2.0 * k[1:, 1:], rtol=1e-15)
    assert np.array_equal(fr.smooth(mean, np.ones((1, 1))), mean)


# ---- the Python layer on the restatement -------------------------------------------
def _image(pixels, pol="stokesIQUV"):
    g = sr.geometry(pixels.shape[0], pol)
    g["shape"] = np.array(pixels.shape[2:])
    return sr.make_image(g, pixels=pixels)


def _blob(pixels, chan, y, x, peak):
    """A plus-shaped blob of five pixels, in Stokes I and, scaled, in Q."""
    for dy, dx, f in ((0, 0, 1.0), (0, 1, 0.5), (0, -1, 0.5), (1, 0, 0.5), (-1, 0, 0.5)):
        pixels[chan, 0, y + dy, x + dx] += peak * f
        pixels[chan, 1, y + dy, x + dx] += 0.1 * peak * f


def _three_blob_image():
    pixels = np.zeros((3, 4, 40, 50))
    for chan in range(3):
        _blob(pixels, chan, 30, 10, 4.0 + chan)   # second in raster order
        _blob(pixels, chan, 5, 40, 2.0)           # first
    # the third moves: its peak is at x = 20, 21, 21 with values 1, 2, 1 -> mean x 20.75,
    # and at y = 20, 20, 21 -> mean y 20.25
    _blob(pixels, 0, 20, 20, 1.0)
    _blob(pixels, 1, 20, 21, 2.0)
    _blob(pixels, 2, 21, 21, 1.0)
    return pixels


def test_find_skycomponents_python_layer():
    pixels = _three_blob_image()
    im = _image(pixels.copy())
    with fr.host_kernels():
        comps = ops.find_skycomponents(im, fwhm=1.0, threshold=0.1, npixels=5)
        labels, n = ops.segment_image(im, fwhm=1.0, threshold=0.1, npixels=5)
    assert np.array_equal(np.asarray(im["pixels"].data), pixels)
    assert n == 3 and isinstance(labels, np.ndarray) and labels.dtype == np.int32
    assert [c.name for c in comps] == ["Segment 0", "Segment 1", "Segment 2"]
    assert all(c.shape == "Point" and c.params == {} for c in comps)
    assert all(c.polarisation_frame == dm.PolarisationFrame("stokesIQUV") for c in comps)
    assert all(np.array_equal(c.frequency, im.frequency.data) for c in comps)
    wcs = im.image_acc.wcs
    xy = [dm.skycoord_to_pixel(c.direction, wcs, 0) for c in comps]
    np.testing.assert_allclose([float(x[0]) for x, _ in xy], [40.0, 20.75, 10.0], atol=1e-6)
    np.testing.assert_allclose([float(y[0]) for _, y in xy], [5.0, 20.25, 30.0], atol=1e-6)
    # flux: the pixel at the rounded mean position, all channels and polarisations
    assert np.array_equal(comps[0].flux, pixels[:, :, 5, 40])
    assert np.array_equal(comps[1].flux, pixels[:, :, 20, 21])
    assert np.array_equal(comps[2].flux, pixels[:, :, 30, 10])
    assert comps[0].flux.shape == (3, 4)
    # and it is the restatement's step 5
    for c, r in zip(comps, fr.find(im, 1.0, 0.1, 5)):
        assert c.direction.ra.rad == r["ra"] and c.direction.dec.rad == r["dec"]
        assert np.array_equal(c.flux, r["flux"]) and c.name == r["name"]


def test_positions_round_half_to_even():
    # peaks of equal weight at x = 10 and 11 (mean 10.5 -> 10) and y = 7 and 8 (7.5 -> 8)
    pixels = np.zeros((2, 1, 20, 30))
    pixels[0, 0, 6:10, 9:13] = 1.0
    pixels[1, 0, 6:10, 9:13] = 1.0
    pixels[0, 0, 7, 10] = 3.0
    pixels[1, 0, 8, 11] = 3.0
    pixels[:, 0, 8, 10] = (0.25, 0.5)
    im = _image(pixels, "stokesI")
    with fr.host_kernels():
        comps = ops.find_skycomponents(im, fwhm=1.0, threshold=0.1, npixels=5)
    assert len(comps) == 1 and np.array_equal(comps[0].flux, [[0.25], [0.5]])


def test_find_skycomponents_errors_and_empty():
    im = _image(np.zeros((1, 1, 16, 16)), "stokesI")
    with fr.host_kernels():
        with pytest.raises(ValueError, match="Failed to find any components"):
            ops.find_skycomponents(im, threshold=1.0)
        labels, n = ops.segment_image(im, threshold=1.0)
        assert n == 0 and labels.shape == (16, 16) and not labels.any()
        bad = np.zeros((1, 1, 16, 16))
        bad[0, 0, 3, 3] = np.inf
        with pytest.raises(ValueError, match="not finite"):
            ops.find_skycomponents(_image(bad, "stokesI"))
        with pytest.raises(ValueError, match="at most 15"):
            ops.find_skycomponents(im, fwhm=12.0)
        with pytest.raises(ValueError, match="float32 or float64"):
            ops.find_skycomponents(_image(np.zeros((1, 1, 8, 8), dtype=np.int32), "stokesI"))


def test_smoothing_joins_and_npixels_drops():
    pixels = np.zeros((1, 1, 24, 24))
    pixels[0, 0, 10, 8] = pixels[0, 0, 10, 12] = 10.0   # three pixels apart
    im = _image(pixels, "stokesI")
    with fr.host_kernels():
        assert ops.segment_image(im, fwhm=1.0, threshold=0.01, npixels=1)[1] == 2
        assert ops.segment_image(im, fwhm=1.0, threshold=0.01, npixels=2)[1] == 0
        labels, n = ops.segment_image(im, fwhm=3.0, threshold=0.01, npixels=5)
        assert n == 1 and labels[10, 10] == 1


# ---- catalogue helpers ----------------------------------------------------------------
def _comp(ra, dec, flux=1.0, nchan=1):
    return dm.SkyComponent(dm.SkyCoord(ra, dec), np.linspace(1e8, 1.2e8, nchan), "c",
                           np.full((nchan, 1), flux), polarisation_frame=dm.PolarisationFrame("stokesI"))


def test_nearest_and_separations():
    # on the equator separations are the differences in ra; on a meridian in dec
    comps = [_comp(0.0, 0.0), _comp(0.03, 0.0), _comp(0.0, -0.01), _comp(0.0, 0.01)]
    home = dm.SkyCoord(0.0, 0.002)
    assert ops.find_nearest_skycomponent_index(home, comps) == 0
    best, sep = ops.find_nearest_skycomponent(dm.SkyCoord(0.0, 0.0051), comps)
    assert best is comps[3] and abs(sep - 0.0049) < 1e-15
    # a tie: the first wins
    assert ops.find_nearest_skycomponent_index(dm.SkyCoord(0.0, 0.0), comps[2:]) == 0
    with pytest.raises(ValueError, match="Catalog is empty"):
        ops.find_nearest_skycomponent_index(home, [])
    d = ops.find_separation_skycomponents(comps)
    want = np.array([[0, 0.03, 0.01, 0.01], [0.03, 0, 0, 0], [0.01, 0, 0, 0.02], [0.01, 0, 0.02, 0]])
    want[1, 2] = want[2, 1] = want[1, 3] = want[3, 1] = np.arccos(np.cos(0.03) * np.cos(0.01))
    np.testing.assert_allclose(d, want, atol=1e-14)
    s = ops.find_separation_skycomponents(comps[:2], comps)
    assert s.shape == (4, 2)
    np.testing.assert_allclose(s, want[:, :2], atol=1e-14)


def test_matches():
    ref = [_comp(0.0, 0.0), _comp(0.1, 0.0), _comp(0.2, 0.0)]
    test = [_comp(0.2 + 2e-8, 0.0), _comp(0.05, 0.0), _comp(1e-8, 0.0), _comp(3e-8, 0.0)]
    for match in (ops.find_skycomponent_matches, ops.find_skycomponent_matches_atomic):
        m = match(test, ref, tol=1e-7)
        assert [(t, r) for t, r, _ in m] == [(0, 2), (2, 0), (3, 0)]
        np.testing.assert_allclose([s for _, _, s in m], [2e-8, 1e-8, 3e-8], rtol=1e-6)
        assert match(test, ref, tol=1.5e-8) == [(2, 0, m[1][2])]
        assert match([], ref) == []
        with pytest.raises(ValueError):
            match(test, [])


def test_select_remove_filter_fit():
    home = dm.SkyCoord(0.0, 0.0)
    comps = [_comp(0.0, 0.0, 1.0), _comp(0.01, 0.0, 3.0), _comp(0.02, 0.0, 2.0), _comp(0.1, 0.0, 5.0)]
    assert ops.select_components_by_separation(home, comps) == comps
    assert ops.select_components_by_separation(home, comps, rmax=0.05, rmin=0.005) == comps[1:3]
    # 0-1 closer than 0.015: 0 is fainter and goes; then 1-2: 2 is fainter and goes
    idx, kept = ops.remove_neighbouring_components(comps, 0.015)
    assert idx == [1, 3] and kept == [comps[1], comps[3]]
    assert ops.remove_neighbouring_components(comps, 0.001)[0] == [0, 1, 2, 3]
    assert ops.filter_skycomponents_by_flux(comps, flux_min=1.0, flux_max=5.0) == comps[1:3]
    assert ops.filter_skycomponents_by_flux(comps) == comps
    c = _comp(0.0, 0.0, 1.0, nchan=5)
    c.flux = (2.0 * (c.frequency / c.frequency[2]) ** -0.7)[:, None]
    assert abs(ops.fit_skycomponent_spectral_index(c) + 0.7) < 1e-12
    assert ops.fit_skycomponent_spectral_index(_comp(0.0, 0.0)) == 0.0
    c.flux = -c.flux
    assert ops.fit_skycomponent_spectral_index(c) == 0.0


def test_exports():
    import ska_sdp_func_python_amd.sky_component as pkg
    for name in ("find_skycomponents", "segment_image", "find_nearest_skycomponent_index",
                 "find_nearest_skycomponent", "find_separation_skycomponents",
                 "find_skycomponent_matches_atomic", "find_skycomponent_matches",
                 "select_components_by_separation", "remove_neighbouring_components",
                 "filter_skycomponents_by_flux", "fit_skycomponent_spectral_index"):
        assert callable(getattr(pkg, name)), name
