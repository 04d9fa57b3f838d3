"""find_skycomponents on the device (csrc/segment.hip) against the host
restatement of tests/findcomp_restatement.py: segment maps, segment counts,
peak values and peak indices must be EQUAL.

The restatement is written from numpy and scipy.ndimage.label (the call that
photutils' detect_sources makes); it is not a run of the reference, whose
astropy 5.2.2 and photutils 1.8.0 are not available where this project is
built: its smoothing and its peaks rest on their documented behaviour (the
restatement's docstring says which lines of the reference each step restates).

Image sizes (findcomp_restatement.SHAPES): 75 x 150 gives three by five of the
kernel's 32 x 32 tiles with a ragged last tile each way; one row; one column;
64 x 96 is whole tiles.

The end-to-end test follows the reference's own acceptance of an image
(tests/imaging/test_imaging.py:93-110).  Its components are inserted and then
restored, so that a centre pixel holds the flux twice; "the faintest peak" of
which the threshold is half is taken to be the faintest restored (Gaussian)
peak, the smallest channel-mean Stokes-I flux: half of the faintest pixel would
leave that component's segment a single pixel, short of npixels = 5.
"""

import functools

import numpy as np
import pytest

import findcomp_restatement as fr
import skycomp_restatement as sr

pytestmark = pytest.mark.gpu

NAMES = [name for name, _ in fr.mask_cases(4, 4)]
# seeds of the smoothing cases, picked on the CPU so that findcomp_restatement.margin_ok holds
SMOOTH_THRESHOLD = 0.3
SMOOTH_SEEDS = {2.0: 11, 3.0: 12, 4.0: 12}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu tests need an MI355X")
    return torch.device("cuda:0")


def on(dev, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def check(dev, planes, threshold, npixels, kernel=None):
    """Device segment_image + segment_peaks of numpy planes == the restatement;
    returns (labels, nlabels)."""
    from ska_sdp_func_python_amd import kernels
    want, n = fr.segment(planes, threshold, npixels, kernel)
    t = on(dev, planes)
    labels, nlabels = kernels.segment_image(t, threshold, npixels, kernel)
    assert str(labels.dtype) == "torch.int32" and labels.is_cuda
    assert nlabels == n
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(t.cpu().numpy(), planes)  # the planes are only read
    values, indices = kernels.segment_peaks(t, labels, nlabels)
    wv, wi = fr.peaks(planes, want, n)
    assert values.shape == (planes.shape[0], n) and str(indices.dtype) == "torch.int64"
    assert np.array_equal(values.cpu().numpy(), wv)
    assert np.array_equal(indices.cpu().numpy(), wi)
    return want, n


@functools.lru_cache(maxsize=None)
def shape_cases(ny, nx):
    return dict(fr.mask_cases(ny, nx))


def valued(mask, seed=5):
    """One channel: 1 + u on the mask, 0 off it (threshold 0.5), u uniform."""
    u = np.random.default_rng(seed).random(mask.shape)
    return np.where(mask, 1.0 + u, 0.0)[None]


# ---- shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(dev, shape, name):
    mask = shape_cases(*shape)[name]
    planes = valued(mask)
    _, n1 = check(dev, planes, 0.5, 1)
    _, n5 = check(dev, planes, 0.5, 5)
    assert n5 <= n1
    if name.startswith("random") and shape == fr.SHAPES[0]:
        # the mask is `pixels > threshold` of the uniform pixels themselves
        fill = int(name[6:]) / 100.0
        pix = np.random.default_rng(77).random((1,) + shape)
        _, n = check(dev, pix, 1.0 - fill, 3)
        assert n > 0


@pytest.mark.parametrize("shape", fr.SHAPES[:1] + fr.SHAPES[3:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_exactly_npixels_kept_one_fewer_dropped(dev, shape):
    mask, kept = fr.bars(*shape, 5)
    _, n = check(dev, valued(mask), 0.5, 5)
    assert n == kept > 10
    _, n = check(dev, valued(mask), 0.5, 4)
    assert n == 2 * kept - 1


def test_pixel_equal_to_threshold_is_excluded(dev):
    ny, nx = fr.SHAPES[0]
    planes = np.zeros((1, ny, nx))
    planes[0, 30:34, 29:35] = 2.0
    planes[0, 30:34, 35] = 1.0                        # equal to the threshold: outside
    planes[0, 30:34, 36] = 2.0                        # so this block is a segment of its own
    planes[0, 40, 10:16] = np.nextafter(1.0, 2.0)     # just above: inside
    labels, n = check(dev, planes, 1.0, 1)
    assert n == 3 and labels[30, 35] == 0 and labels[30, 34] == 1 and labels[30, 36] == 2
    assert np.count_nonzero(labels == 3) == 6


def test_nothing_above_threshold(dev):
    from ska_sdp_func_python_amd import kernels
    from ska_sdp_func_python_amd.sky_component import operations as ops
    ny, nx = fr.SHAPES[0]
    pix = np.random.default_rng(3).random((2, 1, ny, nx))
    labels, n = kernels.segment_image(on(dev, pix[:, 0]), 1.0, 1)
    assert n == 0 and not labels.any().item()
    values, indices = kernels.segment_peaks(on(dev, pix[:, 0]), labels, 0)
    assert values.shape == (2, 0) and indices.shape == (2, 0)
    g = sr.geometry(2, "stokesI")
    g["shape"] = np.array([ny, nx])
    im = sr.make_image(g, pixels=pix, to=lambda p: on(dev, p))
    with pytest.raises(ValueError, match="Failed to find any components"):
        ops.find_skycomponents(im, fwhm=1.0, threshold=1.0, npixels=1)
    labels, n = ops.segment_image(im, fwhm=1.0, threshold=1.0, npixels=1)
    assert n == 0 and labels.is_cuda and labels.shape == (ny, nx) and not labels.any().item()


def test_refusals(dev):
    from ska_sdp_func_python_amd import kernels
    pix = np.zeros((2, 40, 50))
    with pytest.raises(ValueError, match="at most 15"):
        kernels.segment_image(on(dev, pix), 1.0, 1, np.full((17, 17), 1.0 / 289))
    for bad in (np.nan, np.inf, -np.inf):
        p = pix.copy()
        p[1, 39, 49] = bad
        with pytest.raises(ValueError, match="not finite"):
            kernels.segment_image(on(dev, p), 1.0, 1)
    with pytest.raises(ValueError, match="float32 or float64"):
        kernels.segment_image(on(dev, pix.astype(np.int32)), 1.0, 1)


# ---- peaks ----------------------------------------------------------------------------
def test_peak_ties_across_tile_borders(dev):
    ny, nx = fr.SHAPES[0]
    planes = np.zeros((1, ny, nx))
    planes[0, 10, 28:37] = 1.0
    planes[0, 10, [33, 30, 35]] = 4.0     # left and right of the border at x = 32
    planes[0, 28:37, 70] = 1.0
    planes[0, [33, 30], 70] = 5.0         # above and below the border at y = 32
    planes[0, 60:70, 60:70] = -0.0        # a block of zeros of both signs, all equal
    planes[0, 62, 61] = 0.0
    want, n = check(dev, planes + 0.0, 0.5, 1)
    assert n == 2
    from ska_sdp_func_python_amd import kernels
    labels = np.zeros((ny, nx), dtype=np.int32)
    labels[10, 28:37] = 1
    labels[28:37, 70] = 2
    labels[60:70, 60:70] = 3
    values, indices = kernels.segment_peaks(on(dev, planes), on(dev, labels), 3)
    assert np.array_equal(values.cpu().numpy(), [[4.0, 5.0, 0.0]])
    assert np.array_equal(indices.cpu().numpy(), [[10 * nx + 30, 30 * nx + 70, 60 * nx + 60]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_peaks_per_channel(dev, dtype):
    """Five channels with their peaks on different pixels, one of them negative
    over the segments, on a strided view of a cube with two polarisations."""
    from ska_sdp_func_python_amd import kernels
    ny, nx = fr.SHAPES[0]
    rng = np.random.default_rng(21)
    cube = rng.standard_normal((5, 2, ny, nx))
    cube[:, 0] += 1.5
    cube[3, 0] = -np.abs(cube[3, 1]) - 0.1
    cube = cube.astype(dtype)
    planes = cube[:, 0]
    want, n = fr.segment(planes, 1.1, 5)
    assert 3 < n
    t = on(dev, cube)
    labels, nlabels = kernels.segment_image(t[:, 0], 1.1, 5)
    assert nlabels == n and np.array_equal(labels.cpu().numpy(), want)
    values, indices = kernels.segment_peaks(t[:, 0], labels, nlabels)
    wv, wi = fr.peaks(planes, want, n)
    assert np.array_equal(values.cpu().numpy(), wv) and np.array_equal(indices.cpu().numpy(), wi)
    assert (wv[3] < 0).all() and len(set(wi[:, 0])) > 1
    assert np.array_equal(t.cpu().numpy(), cube)


def test_float32_mean_is_formed_in_float32(dev):
    """3 + 2^-24 + 2^-24 is 3 in float32 and above 3 in float64."""
    ny, nx = 40, 70
    p32 = np.zeros((3, ny, nx), dtype=np.float32)
    p32[0, 5:9, 30:36] = 3.0
    p32[1:, 5:9, 30:36] = 2.0 ** -24
    thr = 1.0   # the float32 mean is exactly 1: not above
    assert fr.segment(p32, thr, 1)[1] == 0 and fr.segment(p32.astype(np.float64), thr, 1)[1] == 1
    check(dev, p32, thr, 1)
    check(dev, p32.astype(np.float64), thr, 1)


# ---- smoothing ------------------------------------------------------------------------
@pytest.mark.parametrize("fwhm", sorted(SMOOTH_SEEDS))
@pytest.mark.parametrize("shape", fr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_smoothing(dev, shape, fwhm):
    planes = fr.blobs_image(*shape, 3, SMOOTH_SEEDS[fwhm])
    # only a smoothed value this close to the threshold could come out on the other
    # side of it where the device rounds the window sum in another order
    assert fr.margin_ok(planes, fwhm, SMOOTH_THRESHOLD)
    _, n = check(dev, planes, SMOOTH_THRESHOLD, 5, fr.kernel_of(fwhm))
    assert n >= 1


def test_identity_kernel_is_exact(dev):
    from ska_sdp_func_python_amd import kernels
    planes = fr.blobs_image(*fr.SHAPES[0], 1, 4)
    thr = float(np.sort(planes.ravel())[planes.size // 2])   # a pixel's own value
    a, na = kernels.segment_image(on(dev, planes), thr, 1, np.ones((1, 1)))
    b, nb = kernels.segment_image(on(dev, planes), thr, 1)
    want, n = fr.label_mask(planes[0] > thr, 1)
    assert na == nb == n
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)


# ---- repeatability -------------------------------------------------------------------
def test_repeatable(dev):
    import torch
    from ska_sdp_func_python_amd import kernels
    planes = on(dev, fr.blobs_image(*fr.SHAPES[0], 3, 9) + valued(fr.random_mask(*fr.SHAPES[0], 0.45, 1)))
    k = fr.kernel_of(2.0)
    l1, n1 = kernels.segment_image(planes, 0.8, 2, k)
    v1, i1 = kernels.segment_peaks(planes, l1, n1)
    l2, n2 = kernels.segment_image(planes, 0.8, 2, k)
    v2, i2 = kernels.segment_peaks(planes, l2, n2)
    assert n1 == n2 > 5
    assert torch.equal(l1, l2) and torch.equal(i1, i2)
    assert torch.equal(v1.view(torch.int64), v2.view(torch.int64))


# ---- end to end -----------------------------------------------------------------------
def _inserted_restored(to):
    """A 3-channel IQUV image with 12 components on pixel centres, inserted and
    restored with a beam of 3.5 pixels FWHM; returns (image, components, their
    pixels (x, y), the threshold: half the faintest restored peak)."""
    from ska_sdp_func_python_amd.sky_component import operations as ops
    g = sr.geometry(3, "stokesIQUV")
    ny, nx = 80, 100
    g["shape"] = np.array([ny, nx])
    im = sr.make_image(g, pixels=np.zeros((3, 4, ny, nx)), to=to)
    rng = np.random.default_rng(8)
    positions = [(x, y) for y in (12, 37, 62) for x in (11, 35, 60, 86)]
    # components on five frequencies around the image's three channels (the cubic
    # interpolation in frequency needs four), their flux linear in frequency:
    # a + b c on image channel c
    f0, bw = float(g["frequency"]), float(g["channel_bandwidth"])
    steps = np.arange(-1.0, 4.0)
    a, b = rng.uniform(1.0, 3.0, (12, 1, 4)), rng.uniform(-0.2, 0.2, (12, 1, 4))
    a[:, :, 1:] *= 0.1
    flux = a + b * steps[None, :, None]
    comps = sr.components_at(im, positions, flux, frequency=f0 + bw * steps)
    faintest = float((a + b)[:, 0, 0].min())   # the mean over channels 0, 1, 2
    ops.insert_skycomponent(im, comps)
    ops.restore_skycomponent(im, comps, clean_beam=sr.beam_of_sigma(3.5 / np.sqrt(8.0 * np.log(2.0))))
    return im, comps, positions, 0.5 * faintest


def test_end_to_end(dev):
    import torch
    from ska_sdp_func_python_amd.sky_component import operations as ops
    im, comps, positions, threshold = _inserted_restored(lambda p: on(dev, p))
    pixels = im["pixels"].data
    assert pixels.is_cuda
    before = pixels.clone()
    found = ops.find_skycomponents(im, fwhm=1.0, threshold=threshold, npixels=5)
    assert im["pixels"].data is pixels and pixels.is_cuda and torch.equal(pixels, before)
    assert len(found) == len(comps) == 12
    cellsize = np.deg2rad(abs(im.image_acc.wcs.wcs.cdelt[0]))
    host = pixels.cpu().numpy()
    seen = set()
    for k, comp in enumerate(found):
        nearest = ops.find_nearest_skycomponent_index(comp.direction, comps)
        _, separation = ops.find_nearest_skycomponent(comp.direction, comps)
        assert separation / cellsize < 0.1
        seen.add(nearest)
        x, y = positions[nearest]
        assert comp.name == f"Segment {k}" and isinstance(comp.flux, np.ndarray)
        assert np.array_equal(comp.flux, host[:, :, y, x])
    assert seen == set(range(12))
    # against the restatement, on the same pixels on the host
    g = sr.geometry(3, "stokesIQUV")
    g["shape"] = np.array(host.shape[2:])
    him = sr.make_image(g, pixels=host.copy())
    want = fr.find(him, 1.0, threshold, 5)
    assert len(want) == 12
    for comp, w in zip(found, want):
        assert abs(comp.direction.ra.rad - w["ra"]) <= 1e-12
        assert abs(comp.direction.dec.rad - w["dec"]) <= 1e-12
        assert np.array_equal(comp.flux, w["flux"])
    # numpy in: the same result, numpy out, pixels untouched
    again = ops.find_skycomponents(him, fwhm=1.0, threshold=threshold, npixels=5)
    assert isinstance(him["pixels"].data, np.ndarray) and np.array_equal(him["pixels"].data, host)
    for a, b in zip(again, found):
        assert a.direction == b.direction and np.array_equal(a.flux, b.flux) and a.name == b.name
    dlabels, n = ops.segment_image(im, fwhm=1.0, threshold=threshold, npixels=5)
    hlabels, hn = ops.segment_image(him, fwhm=1.0, threshold=threshold, npixels=5)
    assert n == hn == 12 and dlabels.is_cuda and isinstance(hlabels, np.ndarray)
    assert np.array_equal(dlabels.cpu().numpy(), hlabels)
    assert np.array_equal(hlabels, fr.segment(host[:, 0], threshold, 5)[0])
