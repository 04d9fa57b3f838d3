"""CPU: the facet and channel iterators, scatters and gathers on numpy pixels
against the reference's own results (tests/golden/facets_*.npz;
make_golden_facets.py).  Every comparison of pixels is bit for bit, the signs
of zeros included.

``deconvolution._scatter_channels`` / ``_gather_channels`` now call the public
channel functions: they are held here against a restatement of what they did
before; ``deconvolve_cube`` and ``restore_cube``, which need the device, stay
pinned to the reference's results by tests/test_gpu_clean.py and
tests/test_gpu_mfsclean.py.
"""

import numpy as np
import pytest

from conftest import golden
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd import image
from ska_sdp_func_python_amd.image import deconvolution, iterators
from ska_sdp_func_python_amd.util.array_functions import tukey_filter

import facets_case as C


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module", params=list(C.CASES))
def case(request):
    g = golden(f"facets_{request.param}.npz")
    assert same_bits(g["pixels"], C.case_pixels(request.param))
    return request.param, g


# ---- the goldens ---------------------------------------------------------------------
def test_scatter_matches_the_reference(case):
    name, g = case
    ny, nx, facets, overlap, taper, dtype = C.CASES[name]
    im = C.make_image(g["pixels"].copy())
    subs = image.image_scatter_facets(im, facets=facets, overlap=overlap, taper=taper)
    assert len(subs) == facets * facets
    dy, dx = ny // facets, nx // facets
    for sub, (y, x), crpix in zip(subs, g["origins"], g["crpix"]):
        view = sub["pixels"].data
        assert np.shares_memory(view, im["pixels"].data)
        assert same_bits(view, g["pixels"][..., y:y + dy, x:x + dx])
        assert np.array_equal(sub.image_acc.wcs.wcs.crpix, crpix)
        assert sub.image_acc.polarisation_frame == im.image_acc.polarisation_frame
    assert np.array_equal(im.image_acc.wcs.wcs.crpix, [nx // 2 + 1, ny // 2 + 1, 1.0, 1.0])
    assert list(iterators.image_raster_iter(im, facets=1))[0] is im


def test_gather_matches_the_reference_bit_for_bit(case):
    name, g = case
    ny, nx, facets, overlap, taper, dtype = C.CASES[name]
    im = C.make_image(g["pixels"].copy())
    facet_list = C.facet_images(image.image_scatter_facets(im, facets=facets, overlap=overlap))
    out = image.image_gather_facets(facet_list, im, facets=facets, overlap=overlap, taper=taper)
    assert same_bits(out["pixels"].data, g["gathered"])
    assert out.image_acc.wcs is im.image_acc.wcs
    flat = image.image_gather_facets(facet_list, im, facets=facets, overlap=overlap, taper=taper,
                                     return_flat=True)
    assert same_bits(flat["pixels"].data, g["flat"])
    assert same_bits(im["pixels"].data, g["pixels"])  # a template only
    if name in C.MINUS_ZERO:
        where = C.MINUS_ZERO[name]
        assert np.signbit(g["pixels"][where]) and not np.signbit(out["pixels"].data[where])


def test_the_cases_cover_what_they_claim():
    g = golden("facets_margins.npz")
    assert (g["gathered"][0, 0] == 0.0).sum() == 196
    g = golden("facets_linear_nonsquare.npz")
    assert (g["flat"] == 0.0).any() and (g["gathered"][g["flat"] == 0.0] == 0.0).all()
    assert golden("facets_linear_f32.npz")["gathered"].dtype == np.float32
    assert str(golden("facets_tukey.npz")["taper"]) == "tukey"


def test_tapers_match_the_reference(case):
    name, g = case
    ny, nx, facets, overlap, taper, dtype = C.CASES[name]
    assert same_bits(iterators.taper_1d(taper, ny // facets, overlap), g["taper_y"])
    assert same_bits(iterators.taper_1d(taper, nx // facets, overlap), g["taper_x"])


def test_tukey_filter():
    assert tukey_filter(0.5, 0.5) == 1.0 and tukey_filter(0.0, 0.5) == 0.0
    assert tukey_filter(1.0, 0.5) == 0.0 and tukey_filter(1.5, 0.5) == 1.0
    assert tukey_filter(0.125, 0.5) == 0.5 * (1.0 + np.cos(2.0 * np.pi * (0.125 - 0.25) / 0.5))


# ---- views, WCS, flats ------------------------------------------------------------------
def test_a_facet_is_a_view_of_its_parent():
    im = C.make_image(C.image_pixels(24, 20))
    subs = image.image_scatter_facets(im, facets=2, overlap=1)
    subs[3]["pixels"].data[...] = 7.0
    y, x = 24 // 2 - 1, 20 // 2 - 1
    assert (im["pixels"].data[..., y:y + 12, x:x + 10] == 7.0).all()
    assert (im["pixels"].data == 7.0).sum() == 2 * 2 * 12 * 10
    for r in iterators.image_raster_iter(im, facets=2):
        r["pixels"].data[...] = 1.0
    assert (im["pixels"].data == 1.0).all()


def test_sub_image_wcs_is_a_shifted_deep_copy():
    im = C.make_image(C.image_pixels(26, 22))
    subs = image.image_scatter_facets(im, facets=2, overlap=2)
    # dy = 13, dx = 11, steps 9 and 7, origins 13 - 9 - 2 and 11 - 7 - 2
    assert np.array_equal(subs[0].image_acc.wcs.wcs.crpix, [12.0 - 2, 14.0 - 2, 1.0, 1.0])
    assert np.array_equal(subs[3].image_acc.wcs.wcs.crpix, [12.0 - 9, 14.0 - 11, 1.0, 1.0])
    subs[0].image_acc.wcs.wcs.crval[0] = 99.0
    assert im.image_acc.wcs.wcs.crval[0] == 15.0
    # the sky position of a pixel is the same through either WCS
    world_parent = im.image_acc.wcs.wcs_pix2world(9 + 3, 11 + 4, 0)
    world_facet = subs[3].image_acc.wcs.wcs_pix2world(3, 4, 0)
    assert np.array_equal(world_parent[:2], world_facet[:2])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_make_flat_yields_new_taper_images(dtype):
    g = golden("facets_linear_nonsquare.npz")
    im = C.make_image(C.image_pixels(26, 22, dtype))
    before = im["pixels"].data.copy()
    flats = list(iterators.image_raster_iter(im, facets=2, overlap=2, taper="linear",
                                             make_flat=True))
    want = np.outer(g["taper_y"], g["taper_x"]).astype(dtype)
    assert len(flats) == 4
    for flat in flats:
        data = flat["pixels"].data
        assert not np.shares_memory(data, im["pixels"].data) and data.dtype == np.dtype(dtype)
        assert all(same_bits(data[c, p], want) for c in range(2) for p in range(2))
    assert same_bits(im["pixels"].data, before)
    # an unknown taper is flat; without an overlap make_flat yields the views
    flats = list(iterators.image_raster_iter(im, facets=2, overlap=2, taper="none", make_flat=True))
    assert (flats[0]["pixels"].data == 1.0).all()
    views = list(iterators.image_raster_iter(im, facets=2, overlap=0, make_flat=True))
    assert np.shares_memory(views[0]["pixels"].data, im["pixels"].data)


def test_a_single_facet_with_an_overlap_is_the_image():
    pixels = C.image_pixels(12, 10)
    im = C.make_image(pixels)
    out = image.image_gather_facets([im], im, facets=1, overlap=3, taper="linear")
    assert same_bits(out["pixels"].data, pixels + 0.0)
    flat = image.image_gather_facets([im], im, facets=1, overlap=3, return_flat=True)
    assert same_bits(flat["pixels"].data, np.ones_like(pixels))


# ---- refusals -------------------------------------------------------------------------
def test_the_reference_s_refusals():
    for ny, nx, facets, overlap in golden("facets_refused.npz")["rasters"]:
        im = C.make_image(C.image_pixels(ny, nx))
        with pytest.raises(ValueError):
            image.image_scatter_facets(im, facets=int(facets), overlap=int(overlap))
    im = C.make_image(C.image_pixels(24, 24))
    with pytest.raises(ValueError, match="more raster elements than pixels"):
        image.image_scatter_facets(im, facets=25)
    with pytest.raises(ValueError, match="zero or less"):
        image.image_scatter_facets(im, facets=0)
    with pytest.raises(ValueError, match="zero or greater"):
        image.image_scatter_facets(im, facets=2, overlap=-1)
    with pytest.raises(ValueError, match="too large"):
        image.image_scatter_facets(im, facets=2, overlap=12)
    bad = dm.Image.constructor(C.image_pixels(24, 24), dm.PolarisationFrame(C.POL_FRAME),
                               dm.WCS(4, ["UU", "VV", "STOKES", "FREQ"], [1.0] * 4))
    with pytest.raises(ValueError, match="not canonical"):
        image.image_scatter_facets(bad, facets=2)
    with pytest.raises(ValueError, match="not canonical"):
        image.image_gather_facets([], bad, facets=2)


def test_deviations_from_the_reference():
    # the y origin is checked like the x origin: three facets with an overlap
    # of 3 fit 30 pixels (8 .. 26) but not 60 (13 .. 61)
    assert len(image.image_scatter_facets(C.make_image(C.image_pixels(30, 30)), facets=3,
                                          overlap=3)) == 9
    with pytest.raises(ValueError, match="starting point 13"):
        image.image_scatter_facets(C.make_image(C.image_pixels(30, 60)), facets=3, overlap=3)
    with pytest.raises(ValueError, match="starting point 13"):
        image.image_scatter_facets(C.make_image(C.image_pixels(60, 30)), facets=3, overlap=3)
    # a step of zero or less
    im = C.make_image(C.image_pixels(24, 24))
    with pytest.raises(ValueError, match="no step"):
        image.image_scatter_facets(im, facets=2, overlap=6)
    with pytest.raises(ValueError, match="no step"):
        image.image_scatter_facets(im, facets=2, overlap=7)
    # the facets given to the gather
    subs = image.image_scatter_facets(im, facets=2)
    with pytest.raises(ValueError, match="facets given"):
        image.image_gather_facets(subs[:3], im, facets=2)
    single = [C.make_image(s["pixels"].data.astype(np.float32)) for s in subs]
    with pytest.raises(ValueError, match="agree with the image"):
        image.image_gather_facets(single, im, facets=2)
    short = [C.make_image(s["pixels"].data[..., :11]) for s in subs]
    with pytest.raises(ValueError, match="is expected"):
        image.image_gather_facets(short, im, facets=2)
    assert same_bits(image.image_gather_facets(subs, im, facets=2)["pixels"].data,
                     im["pixels"].data + 0.0)


# ---- channels -------------------------------------------------------------------------
def cube(nchan=6, dtype="float64"):
    return C.make_image(C.image_pixels(9, 7, dtype, nchan=nchan))


def old_scatter_channels(im):
    """What deconvolution._scatter_channels did before the public function."""
    out = []
    for chan in range(im["pixels"].data.shape[0]):
        wcs = im.image_acc.wcs.deepcopy()
        wcs.wcs.crval[3] += chan * wcs.wcs.cdelt[3]
        out.append(dm.Image.constructor(data=im["pixels"].data[chan:chan + 1], wcs=wcs,
                                        polarisation_frame=im.image_acc.polarisation_frame))
    return out


def same_image(a, b):
    wa, wb = a.image_acc.wcs.wcs, b.image_acc.wcs.wcs
    return same_bits(a["pixels"].data, b["pixels"].data) and \
        all(np.array_equal(getattr(wa, k), getattr(wb, k)) for k in ("crpix", "crval", "cdelt")) \
        and wa.ctype == wb.ctype and a.attrs.keys() == b.attrs.keys() and \
        a.image_acc.polarisation_frame == b.image_acc.polarisation_frame


def test_scatter_channels_default_is_one_image_per_channel():
    im = cube()
    got = image.image_scatter_channels(im)
    want = old_scatter_channels(im)
    assert len(got) == 6 and all(same_image(a, b) for a, b in zip(got, want))
    assert all(same_image(a, b) for a, b in zip(deconvolution._scatter_channels(im), want))
    assert all(np.shares_memory(s["pixels"].data, im["pixels"].data) for s in got)
    assert image.image_scatter_channels(None) is None
    assert deconvolution._scatter_channels(None) is None


@pytest.mark.parametrize("subimages", [1, 2, 3, 6])
def test_scatter_channels_in_equal_blocks(subimages):
    im = cube()
    blocks = image.image_scatter_channels(im, subimages=subimages)
    width = 6 // subimages
    assert len(blocks) == subimages
    for b, block in enumerate(blocks):
        data = block["pixels"].data
        assert data.shape == (width, 2, 9, 7) and np.shares_memory(data, im["pixels"].data)
        assert same_bits(data, im["pixels"].data[b * width:(b + 1) * width])
        assert np.array_equal(block.frequency.data,
                              im.frequency.data[b * width:(b + 1) * width])
    back = image.image_gather_channels(blocks)
    assert same_bits(back["pixels"].data, im["pixels"].data)
    assert np.array_equal(back.frequency.data, im.frequency.data)


def test_scatter_channels_refuses_blocks_that_do_not_divide():
    for subimages in (4, 5, 7, 0, -1):
        with pytest.raises(ValueError, match="does not divide"):
            image.image_scatter_channels(cube(), subimages=subimages)


def test_gather_channels_keeps_the_first_image_s_wcs_and_attrs():
    im = cube()
    parts = image.image_scatter_channels(im)
    parts[0].attrs["clean_beam"] = {"bmaj": 1.0, "bmin": 0.5, "bpa": 0.0}
    out = image.image_gather_channels(parts)
    assert out.image_acc.wcs is parts[0].image_acc.wcs
    assert out.attrs["clean_beam"] == {"bmaj": 1.0, "bmin": 0.5, "bpa": 0.0}
    assert same_image(out, deconvolution._gather_channels(parts))
    assert same_bits(out["pixels"].data, im["pixels"].data)


@pytest.mark.parametrize("subimages", [1, 2, 3, 6])
def test_channel_iter_moves_crpix(subimages):
    im = cube()
    blocks = list(iterators.image_channel_iter(im, subimages=subimages))
    width = 6 // subimages
    assert len(blocks) == subimages
    for b, block in enumerate(blocks):
        assert np.shares_memory(block["pixels"].data, im["pixels"].data)
        assert same_bits(block["pixels"].data, im["pixels"].data[b * width:(b + 1) * width])
        assert block.image_acc.wcs.wcs.crpix[3] == 1.0 - b * width
        assert block.image_acc.wcs.wcs.crval[3] == C.F0
    with pytest.raises(AssertionError, match="More subimages"):
        list(iterators.image_channel_iter(im, subimages=7))
    with pytest.raises(AssertionError, match="does not match"):
        list(iterators.image_channel_iter(im, subimages=4))
