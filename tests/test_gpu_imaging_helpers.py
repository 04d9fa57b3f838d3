"""GPU tests of csrc/imgsum.hip through kernels.sum_planes and kernels.peak_abs,
and of imaging/imaging_helpers.py and the device branches of imaging/base.py on
device tensors.

Every comparison is bitwise, the signs of zeros included, against numpy doing
the same operations in the same order: for float64 that is the reference's own
arithmetic (the numpy paths, which tests/test_imaging_helpers_cpu.py holds
against the reference's fixtures); a float32 weighted sum is the float64 result
rounded once, which is what the kernel documents.
"""

import functools

import numpy as np
import pytest
import torch

from conftest import golden
from ska_sdp_func_python_amd import kernels
from ska_sdp_func_python_amd.image.gather_scatter import image_scatter_facets
from ska_sdp_func_python_amd.imaging import base, imaging_helpers as ih

import imghelp_case as C

pytestmark = pytest.mark.gpu

# 35: the odd planes of a cube are aligned to 8 bytes only (float32: to 4);
# 4096, 4097: a whole number of groups, and one element in a tail group;
# 257 * 263: more than one block
NPIX = [1, 3, 35, 4096, 4097, 257 * 263]


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())  # a copy: the cached cases are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 16: np.int64}[a.dtype.itemsize])


def same_bits(got, want):
    """A device tensor against a numpy array of the same dtype, bit for bit."""
    assert isinstance(got, torch.Tensor) and got.is_cuda
    got = got.detach().cpu().numpy()
    want = np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(_bits(got), _bits(want))


# ---- sum_planes, weighted ------------------------------------------------------------
def weighted_sum(x, w, sumwt, normalise, dtype):
    """numpy's `acc += w[n][:, None] * x[n]` over the list in float64, then
    normalise_sumwt's division or zeroing, then one rounding to dtype."""
    acc = np.zeros(x[0].shape)
    with np.errstate(invalid="ignore"):
        for n in range(len(x)):
            acc += w[n][:, None] * x[n].astype(np.float64)
    if normalise:
        for p in range(acc.shape[0]):
            acc[p] = acc[p] / sumwt[p] if sumwt[p] > 0.0 else 0.0
    return acc.astype(dtype)


@functools.lru_cache(maxsize=None)
def weighted_case(npix, nplane, ncube, dtype):
    """Inputs with -0.0 in every fourth pixel; weights with 0, 1 and -1 among
    normal deviates of either sign; sumwt their sum in list order.  With six
    planes, plane 2 has sumwt 0 and a NaN in its inputs and plane 4 a negative
    sumwt: both must come out as +0.0."""
    rng = np.random.default_rng(100000 * ncube + 1000 * nplane + npix)
    x = rng.normal(size=(ncube, nplane, npix)).astype(dtype)
    x.reshape(-1)[::4] = -0.0
    w = rng.normal(size=(ncube, nplane))
    w.flat[::3] = 0.0
    w.flat[1::5] = 1.0
    w.flat[2::7] = -1.0
    sumwt = np.zeros(nplane)
    for n in range(ncube):
        sumwt += w[n]
    sumwt = np.where(sumwt == 0.0, 0.5, np.abs(sumwt))
    if nplane == 6:
        sumwt[2] = 0.0
        sumwt[4] = -1.5
        x[0, 2, npix // 2] = np.nan
    want = {norm: weighted_sum(x, w, sumwt, norm, dtype) for norm in (True, False)}
    for a in (x, w, sumwt, want[True], want[False]):
        a.setflags(write=False)
    return x, w, sumwt, want


@pytest.mark.parametrize("normalise", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("ncube", [1, 2, 17])
@pytest.mark.parametrize("nplane", [1, 6])
@pytest.mark.parametrize("npix", NPIX)
def test_sum_planes_weighted_matches_numpy_bit_for_bit(npix, nplane, ncube, dtype, normalise):
    x, w, sumwt, want = weighted_case(npix, nplane, ncube, dtype)
    ins = [_t(x[n]) for n in range(ncube)]
    if npix % 2 and nplane > 1:
        assert ins[0][1].data_ptr() % 16
    got = kernels.sum_planes(ins, w, sumwt if normalise else None, normalise=normalise)
    if normalise or nplane == 1:
        assert same_bits(got, want[normalise])
    else:
        # the NaN of plane 2 comes through; which NaN is the processor's choice
        nan = np.isnan(want[False])
        assert nan[2].sum() == 1 and nan.sum() == 1
        assert np.array_equal(np.isnan(got.cpu().numpy()), nan)
        assert same_bits(torch.nan_to_num(got, nan=0.0), np.nan_to_num(want[False], nan=0.0))
    if normalise and nplane == 6:
        zero = got[[2, 4]].cpu().numpy()
        assert not zero.any() and not np.signbit(zero).any()
    for n in range(ncube):
        assert same_bits(ins[n], x[n])


def test_sum_planes_zeroes_a_single_plane_without_weight_whatever_it_sums():
    x = np.full((3, 1, 37), np.nan)
    got = kernels.sum_planes([_t(a) for a in x], np.ones((3, 1)), np.zeros(1))
    assert same_bits(got, np.zeros((1, 37)))


def test_sum_planes_takes_image_cubes_and_copies_strided_inputs():
    rng = np.random.default_rng(7)
    x = rng.normal(size=(3, 2, 3, 5, 14))
    w = rng.normal(size=(3, 2, 3))
    sumwt = np.abs(w.sum(0)) + 0.1
    ins = [_t(x[0]), _t(x[1]), _t(x[2])]
    wide = torch.zeros((2, 3, 5, 28), dtype=torch.float64, device=_dev())
    wide[..., ::2] = ins[1]
    ins[1] = wide[..., ::2]
    assert not ins[1].is_contiguous()
    got = kernels.sum_planes(ins, w, sumwt)
    want = weighted_sum(x.reshape(3, 6, 70), w.reshape(3, 6), sumwt.reshape(6), True, np.float64)
    assert same_bits(got, want.reshape(2, 3, 5, 14))


def test_sum_planes_grid_strides():
    """More groups than one pass of the grid holds, and more planes than it has rows."""
    rng = np.random.default_rng(8)
    npix = (1 << 22) + 2051
    x = rng.normal(size=(2, 1, npix))
    w = np.array([[0.75], [-1.25]])
    got = kernels.sum_planes([_t(x[0]), _t(x[1])], w, np.array([2.0]))
    assert same_bits(got, weighted_sum(x, w, np.array([2.0]), True, np.float64))
    x = rng.normal(size=(2, 9001, 3)).astype(np.float32)
    w = rng.normal(size=(2, 9001))
    sumwt = np.abs(w[0] + w[1])
    got = kernels.sum_planes([_t(x[0]), _t(x[1])], w, sumwt)
    assert same_bits(got, weighted_sum(x, w, sumwt, True, np.float32))


# ---- sum_planes, plain -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_case(npix, ncube, dtype):
    rng = np.random.default_rng(10 * npix + ncube)
    x = rng.normal(size=(ncube, npix))
    if np.dtype(dtype).kind == "c":
        x = x + 1j * rng.normal(size=(ncube, npix))
    x = x.astype(dtype)
    x.real[:, ::4] = -0.0
    want = x[0].copy()
    for n in range(1, ncube):
        want += x[n]
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("alias", [False, True], ids=["new", "onto_first"])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128, np.float32, np.float64],
                         ids=["c64", "c128", "f32", "f64"])
@pytest.mark.parametrize("ncube", [1, 2, 5])
@pytest.mark.parametrize("npix", [1, 3, 35, 4097, 257 * 263])
def test_sum_planes_plain_matches_numpy_bit_for_bit(npix, ncube, dtype, alias):
    x, want = plain_case(npix, ncube, dtype)
    cube = _t(x)
    ins = [cube[n] for n in range(ncube)]
    got = kernels.sum_planes(ins, out=ins[0] if alias else None)
    assert (got is ins[0]) == alias
    assert same_bits(got, want)
    for n in range(0 if not alias else 1, ncube):
        assert same_bits(ins[n], x[n])


def test_sum_planes_refuses_what_it_cannot_do():
    buf = torch.zeros(300, dtype=torch.float64, device=_dev())
    a, b = buf[0:100], buf[150:250]
    w = np.ones((2, 1))
    with pytest.raises(ValueError, match="overlaps"):
        kernels.sum_planes([a, b], out=buf[50:150])
    with pytest.raises(ValueError, match="overlaps"):
        kernels.sum_planes([a, b], out=b)          # only the first entry may be the output
    with pytest.raises(ValueError, match="overlaps"):
        kernels.sum_planes([a.view(1, 100), b.view(1, 100)], w, np.ones(1), out=a.view(1, 100))
    with pytest.raises(ValueError):
        kernels.sum_planes([a, buf[0:99]])
    with pytest.raises(ValueError):
        kernels.sum_planes([a, b.to(torch.float32)])
    with pytest.raises(ValueError):
        kernels.sum_planes([a.cpu(), b.cpu()])
    with pytest.raises(ValueError):
        kernels.sum_planes([a.view(1, 100), b.view(1, 100)], w)      # normalising needs sumwt
    with pytest.raises(ValueError):
        kernels.sum_planes([a.view(1, 100), b.view(1, 100)], np.ones((3, 1)), np.ones(1))
    with pytest.raises(ValueError):
        kernels.sum_planes([a.to(torch.complex128)] * 2, w, np.ones(1))
    with pytest.raises(ValueError):
        kernels.sum_planes([])
    assert kernels.SUM_PLANES_MAX == 4096
    assert not buf.any()


# ---- peak_abs ----------------------------------------------------------------------------
def peak_of(x, mode):
    """numpy.max(|moment 0 / nchan|), the moment summed from +0.0 in channel
    order in float64, or numpy.max(|x[nchan // 2]|)."""
    x = np.asarray(x, dtype=np.float64)
    if mode == "refchan":
        return np.max(np.abs(x[x.shape[0] // 2]))
    acc = np.zeros(x.shape[1:])
    for c in range(x.shape[0]):
        acc += x[c]
    return np.max(np.abs(acc / x.shape[0]))


SHAPES = {"small": (3, 2, 5, 7), "one": (1, 1, 1, 1), "blocks": (2, 4, 257, 263)}
# (pol, y, x) of the peak; for "blocks" as float32 a row holds 65 groups and a
# tail group of 3, and the last block starts in the last row at x = 232
PLACES = {
    "small": {"first": (0, 0, 0), "last": (1, 4, 6), "tail": (0, 2, 6)},
    "one": {"first": (0, 0, 0)},
    "blocks": {"first": (0, 0, 0), "last": (3, 256, 262), "tail": (1, 100, 261),
               "last_block": (3, 256, 240)},
}
PEAK_CASES = [(s, p) for s in SHAPES for p in PLACES[s]]


@functools.lru_cache(maxsize=None)
def background(shape_name, dtype):
    x = (0.1 * np.random.default_rng(5).normal(size=SHAPES[shape_name])).astype(dtype)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("mode", ["moment0", "refchan"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
@pytest.mark.parametrize("shape_name,place", PEAK_CASES)
def test_peak_abs_finds_the_peak_wherever_it_is(shape_name, place, sign, dtype, mode):
    x = background(shape_name, dtype).copy()
    pol, y, col = PLACES[shape_name][place]
    x[:, pol, y, col] = sign * (5.0 + 0.375 * np.arange(x.shape[0]))
    want = peak_of(x, mode)
    assert want > 4.0
    got, flags = kernels.peak_abs(_t(x), mode)
    assert isinstance(got, float) and flags == 0
    assert np.float64(got).tobytes() == np.float64(want).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_peak_abs_sums_the_channels(dtype):
    x = background("small", dtype).copy()
    x[:, 1, 3, 3] = (5.0, 0.0, 4.0)      # the peak exists only in the channel sum
    assert kernels.peak_abs(_t(x), "moment0") == (float(peak_of(x, "moment0")), 0)
    assert peak_of(x, "moment0") == 3.0
    assert kernels.peak_abs(_t(x), "refchan") == (float(peak_of(x, "refchan")), 0)
    assert peak_of(x, "refchan") < 1.0
    two = background("blocks", dtype).copy()
    two[1] = -two[0]                     # the channels cancel
    assert kernels.peak_abs(_t(two), "moment0") == (0.0, 0)
    assert kernels.peak_abs(_t(two), "refchan") == (float(peak_of(two, "refchan")), 0)
    zero = np.zeros(SHAPES["blocks"], dtype=dtype)
    zero[0, 0, 0, ::2] = -0.0
    assert kernels.peak_abs(_t(zero), "moment0") == (0.0, 0)
    assert kernels.peak_abs(_t(zero), "refchan") == (0.0, 0)


def test_peak_abs_reports_nan():
    x = background("small", np.float64).copy()
    x[0, 1, 4, 6] = np.nan               # not the reference channel
    peak, flags = kernels.peak_abs(_t(x), "moment0")
    assert flags & kernels.PEAK_NAN_INPUT
    assert kernels.peak_abs(_t(x), "refchan") == (float(peak_of(x, "refchan")), 0)
    x[1, 0, 0, 0] = np.nan               # the reference channel
    peak, flags = kernels.peak_abs(_t(x), "refchan")
    assert np.isnan(peak) and flags == kernels.PEAK_NAN_INPUT
    y = background("small", np.float64).copy()
    y[0, 0, 1, 1], y[2, 0, 1, 1] = np.inf, -np.inf
    peak, flags = kernels.peak_abs(_t(y), "moment0")
    assert flags == kernels.PEAK_NAN_MEAN
    assert kernels.peak_abs(_t(y), "refchan") == (float(peak_of(y, "refchan")), 0)


def test_peak_abs_grid_strides():
    rng = np.random.default_rng(9)
    x = rng.normal(size=(1, 1, 2049, 2050))
    x[0, 0, 2048, 2049] = -11.0
    assert kernels.peak_abs(_t(x), "moment0") == (11.0, 0)
    x[0, 0, 2048, 2049] = 0.0
    assert kernels.peak_abs(_t(x), "refchan") == (float(np.max(np.abs(x))), 0)


@pytest.mark.parametrize("mode", ["moment0", "refchan"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_peak_abs_reads_facet_views_where_they_lie(dtype, mode):
    rng = np.random.default_rng(10)
    pixels = _t(rng.normal(size=(3, 2, 32, 32)).astype(dtype))
    host = pixels.cpu().numpy()
    im = C.make_image(pixels)
    facets = image_scatter_facets(im, facets=2, overlap=2)
    views = [f["pixels"].data for f in facets]
    views.append(pixels[:, :, 1:30, 3:28])           # rows that start at an odd element
    views.append(pixels[1:, 1:, 5:6, 7:8])           # one pixel of a view
    assert any(v.data_ptr() % 16 for v in views)
    peaks = []
    for v in views:
        assert not v.is_contiguous() and v.data_ptr() != pixels.data_ptr()
        got = kernels.peak_abs(v, mode)
        assert got == kernels.peak_abs(v.contiguous(), mode)
        assert got == (float(peak_of(v.cpu().numpy(), mode)), 0)
        peaks.append(got[0])
    assert len(set(peaks)) > 2                       # the views see different peaks
    assert np.array_equal(_bits(pixels.cpu().numpy()), _bits(host))


def test_peak_abs_refuses_what_it_cannot_do():
    x = torch.zeros((2, 2, 4, 6), dtype=torch.float64, device=_dev())
    with pytest.raises(ValueError):
        kernels.peak_abs(x[..., ::2])
    with pytest.raises(ValueError):
        kernels.peak_abs(x[0])
    with pytest.raises(ValueError):
        kernels.peak_abs(x, "moment1")
    with pytest.raises(ValueError):
        kernels.peak_abs(x.to(torch.complex64))
    with pytest.raises(ValueError):
        kernels.peak_abs(x.cpu())


# ---- the public functions on device tensors ----------------------------------------------------
@pytest.mark.parametrize("name", [n for n in C.INVERT_CASES if n != "one"])
def test_sum_invert_results_on_the_device_gives_numpys_bits(name):
    g = golden("imghelp_sum.npz")
    image_list = C.invert_list(name, convert=_t)
    im, sumwt = ih.sum_invert_results(image_list)
    assert same_bits(im["pixels"].data, g[f"invert_{name}_pixels"])
    assert isinstance(sumwt, np.ndarray) and np.array_equal(_bits(sumwt), _bits(g[f"invert_{name}_sumwt"]))
    assert im.attrs["clean_beam"] == C.CLEAN_BEAM
    assert im.image_acc.polarisation_frame == image_list[0][0].image_acc.polarisation_frame
    for entry, b in zip(image_list, C.invert_case(name)):
        assert entry is None or (same_bits(entry[0]["pixels"].data, b[0])
                                 and np.array_equal(_bits(entry[1]), _bits(b[1])))


def test_sum_invert_results_on_the_device_float32_and_a_list_of_one():
    entries = [e for e in C.invert_case("negative")]
    image_list = C.invert_list("negative", convert=lambda a: _t(a.astype(np.float32)))
    im, sumwt = ih.sum_invert_results(image_list)
    x = np.stack([e[0].astype(np.float32).reshape(-1, C.NY * C.NX) for e in entries])
    w = np.stack([e[1].reshape(-1) for e in entries])
    want = weighted_sum(x, w, sumwt.reshape(-1), True, np.float32)
    assert same_bits(im["pixels"].data, want.reshape(C.NCHAN, C.NPOL, C.NY, C.NX))
    one = C.invert_list("one", convert=_t)
    im, sumwt = ih.sum_invert_results(one)
    assert sumwt is one[0][1] and im is not one[0][0]
    assert im["pixels"].data.data_ptr() != one[0][0]["pixels"].data.data_ptr()
    assert same_bits(im["pixels"].data, C.invert_case("one")[0][0])


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64], ids=["c128", "c64"])
def test_sum_predict_results_on_the_device_sums_onto_the_first_entry(dtype):
    host = C.predict_list(dtype=dtype)
    others = [None if r is None else r["vis"].data.copy() for r in host]
    want = ih.sum_predict_results(host)["vis"].data
    if dtype == np.complex128:
        assert np.array_equal(_bits(want), _bits(golden("imghelp_sum.npz")["predict_vis"]))
    results = C.predict_list(dtype=dtype, convert=_t)
    first = results[1]["vis"].data
    summed = ih.sum_predict_results(results)
    assert summed is results[1] and summed["vis"].data is first
    assert same_bits(first, want)
    for r, b in zip(results[2:], others[2:]):
        assert r is None or same_bits(r["vis"].data, b)
    mismatch = [C.make_vis("low"), C.make_vis("mid")]
    for v in mismatch:
        v["vis"].data = _t(v["vis"].data)
    with pytest.raises(AssertionError):
        ih.sum_predict_results(mismatch)


@pytest.mark.parametrize("name", list(C.THRESHOLD_CASES))
def test_threshold_list_on_the_device_gives_numpys_value(name):
    images, threshold, fraction, moment0 = C.THRESHOLD_CASES[name]
    image_list = C.threshold_list_input(images, convert=_t)
    got = ih.threshold_list(image_list, threshold, fraction, use_moment0=moment0)
    want = golden("imghelp_threshold.npz")[name]
    assert np.float64(got).tobytes() == want.tobytes()
    for im, b in zip(image_list, C.threshold_images(images)):
        assert same_bits(im["pixels"].data, b)


@pytest.mark.parametrize("moment0", [True, False], ids=["moment0", "refchan"])
def test_threshold_list_on_facet_views_and_nan(moment0):
    rng = np.random.default_rng(12)
    host = rng.normal(size=(3, 2, 32, 32))
    want = ih.threshold_list(image_scatter_facets(C.make_image(host.copy()), facets=2, overlap=2),
                             0.0, 0.25, use_moment0=moment0)
    pixels = _t(host)
    facets = image_scatter_facets(C.make_image(pixels), facets=2, overlap=2)
    assert all(not f["pixels"].data.is_contiguous() for f in facets)
    got = ih.threshold_list(facets, 0.0, 0.25, use_moment0=moment0)
    assert np.float64(got).tobytes() == np.float64(want).tobytes()
    assert same_bits(pixels, host)
    if moment0:
        pixels[0, 1, 20, 20] = np.nan                 # in the last facet only
        with pytest.raises(AssertionError, match="NaNs present in image data"):
            ih.threshold_list(facets, 0.0, 0.25, use_moment0=True)


def test_base_functions_take_device_uvw():
    g = golden("imghelp_image.npz")
    vis = C.make_vis("mid")
    vis["uvw"].data = _t(vis["uvw"].data)
    im = base.create_image_from_visibility(vis, npixel=64)
    assert np.array_equal(_bits(np.array(im.image_acc.wcs.wcs.cdelt)), _bits(g["default_cdelt"]))
    ga = golden("imghelp_advise.npz")
    advice = base.advise_wide_field(vis, facets=4, verbose=False)
    for key in ("maximum_baseline", "maximum_w", "cellsize", "npixels", "vis_slices_image"):
        assert np.asarray(advice[key]) == ga[f"mid_f4_{key}"], key
    uvw, dl, dm_ = C.recentre_input()
    got = base.visibility_recentre(_t(uvw), dl, dm_)
    assert same_bits(got, ga["recentre"])
