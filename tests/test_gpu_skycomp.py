"""GPU tests of the sky-component image operations (csrc/skycomp.hip through
kernels.skycomp_* and sky_component/operations.py) against the reference's
outputs (tests/golden/skycomp_*.npz) and the sequential numpy restatements
(tests/skycomp_restatement.py).  Images are 83 x 61.

Bounds.  insert: numpy.array_equal -- every pixel adds its terms in component
order with numpy's roundings.  Voronoi labels: equal.  restore: in every
(chan, pol) plane max|out - ref| <= 1e-12 sum_c |flux_c|: a term's error is at
most |flux| (g |arg| few 2^-53 + ulp) with g |arg| <= 1/e, a few 1e-16 per
term, plus ncomp 2^-53 for the sum; 1e-12 leaves three to four decades over
that, and a misplaced or transposed component errs by O(|flux|)."""

import numpy as np
import pytest
import torch

import skycomp_restatement as R

pytestmark = pytest.mark.gpu

INSERT_CASES = ["nearest", "sinc", "lanczos", "pswf", "lanczos_bw", "freq5", "nearest_off", "single"]
RESTORE_CASES = ["single", "iquv", "freq5"]
RESTORE_TOL = 1e-12


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev())


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _both(run, geometry, dtype=np.float64, on_device=True):
    """``run(im)`` on the GPU and, with the kernels replaced by the sequential
    restatements, on the host: (GPU pixels, restatement pixels)."""
    im = R.make_image(geometry, dtype=dtype, to=_t if on_device else None)
    run(im)
    ref = R.make_image(geometry, dtype=dtype)
    with R.host_kernels():
        run(ref)
    got = _np(im["pixels"].data)
    assert got.dtype == dtype and ref["pixels"].data.dtype == dtype
    assert not np.array_equal(ref["pixels"].data, R.start_pixels(*got.shape, dtype=dtype))
    return got, ref["pixels"].data


def _insert_case(g):
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    comps = R.make_components(g)
    return lambda im: insert_skycomponent(im, comps, insert_method=str(g["method"]),
                                          bandwidth=float(g["bandwidth"]), support=int(g["support"]))


def _beam(g):
    return dict(zip(("bmaj", "bmin", "bpa"), (float(v) for v in g["clean_beam"])))


# ---- 1. insert goldens, bit equality ---------------------------------------------
@pytest.mark.parametrize("on_device", [True, False])
@pytest.mark.parametrize("tag", INSERT_CASES)
def test_insert_golden_is_bit_equal(tag, on_device):
    g = R.load(f"insert_{tag}")
    im = R.make_image(g, to=_t if on_device else None)
    assert _insert_case(g)(im) is im
    assert isinstance(im["pixels"].data, torch.Tensor) == on_device
    assert np.array_equal(_np(im["pixels"].data), g["out_pixels"])


def test_insert_float32_pixels_are_bit_equal():
    g = R.load("insert_lanczos")
    got, ref = _both(_insert_case(g), g, dtype=np.float32)
    assert np.array_equal(got, ref)
    # float32 pixels round after every add: not the float64 result rounded once
    assert not np.array_equal(ref, g["out_pixels"].astype(np.float32))


# ---- 2. order of addition -------------------------------------------------------
@pytest.mark.parametrize("max_pairs", [None, 64])
def test_insert_adds_in_component_order(max_pairs, monkeypatch):
    """300 Lanczos components on three pixel positions whose fluxes cycle
    through 1e16, 1 and -1e16 (times random factors): any other order of
    addition, or an atomic sum, gives other bits.  With at most 64 (tile,
    component) pairs per launch the components go in a few dozen launches."""
    from ska_sdp_func_python_amd import kernels
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    if max_pairs:
        monkeypatch.setattr(kernels.skycomp, "SKYCOMP_MAX_PAIRS", max_pairs)
    rng = np.random.default_rng(11)
    geometry = R.geometry(1, "stokesIQUV")
    pos = np.array([(20.3, 30.7), (23.6, 33.4), (40.45, 47.55)])[np.arange(300) % 3]
    scale = np.array([1e16, 1.0, -1e16])[(np.arange(300) // 3) % 3]
    flux = scale[:, None, None] * rng.uniform(0.5, 1.5, (300, 1, 4))
    im0 = R.make_image(geometry)
    comps = R.components_at(im0, pos, flux)
    got, ref = _both(lambda im: insert_skycomponent(im, comps, insert_method="Lanczos"), geometry)
    assert np.array_equal(got, ref)
    shuffled = R.make_image(geometry)
    with R.host_kernels():
        insert_skycomponent(shuffled, comps[::-1], insert_method="Lanczos")
    assert not np.array_equal(shuffled["pixels"].data, ref)


# ---- 3. tile edges -----------------------------------------------------------------
def test_insert_lattice_crosses_every_tile_edge():
    """PSWF components every 7 pixels with fractional offsets (.3, .7) over the
    whole interior: their 16-pixel windows cross every boundary of any tile
    size up to 64."""
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    rng = np.random.default_rng(12)
    geometry = R.geometry(3, "stokesIQUV")
    pos = R.lattice()
    flux = rng.uniform(-5.0, 5.0, (len(pos), 1, 4))
    comps = R.components_at(R.make_image(geometry), pos, flux, frequency=[1.0e8])
    got, ref = _both(lambda im: insert_skycomponent(im, comps, insert_method="PSWF"), geometry)
    assert len(pos) == 70 and np.array_equal(got, ref)


# ---- 4. grid limits -------------------------------------------------------------
def test_insert_70000_nearest_components():
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    rng = np.random.default_rng(13)
    geometry = R.geometry(1, "stokesI")
    n = 70_000
    pos = np.stack([rng.uniform(-3.0, R.NX + 2.0, n), rng.uniform(-3.0, R.NY + 2.0, n)], 1)
    flux = rng.uniform(-1.0, 1.0, (n, 1, 1)) * 10.0 ** rng.integers(-6, 7, (n, 1, 1))
    comps = R.components_at(R.make_image(geometry), pos, flux)
    got, ref = _both(lambda im: insert_skycomponent(im, comps), geometry)
    assert np.array_equal(got, ref)


# ---- 5. restore: goldens and pruning ---------------------------------------------
def _assert_restored(got, ref, flux, what):
    """``flux`` [ncomp, nchan, npol] as added to the image's planes."""
    bound = RESTORE_TOL * np.abs(flux).sum(axis=0)
    err = np.abs(got - ref).max(axis=(2, 3))
    print(f"\n  restore {what}: max error / sum|flux| per plane = {(err / bound * RESTORE_TOL).max():.2e}")
    assert got.shape == ref.shape and np.all(err <= bound)


@pytest.mark.parametrize("on_device", [True, False])
@pytest.mark.parametrize("tag", RESTORE_CASES)
def test_restore_golden(tag, on_device):
    from ska_sdp_func_python_amd.sky_component import restore_skycomponent
    from ska_sdp_func_python_amd.sky_component.operations import _image_flux
    g = R.load(f"restore_{tag}")
    im = R.make_image(g, to=_t if on_device else None)
    comps = R.make_components(g)
    cb = _beam(g)
    assert restore_skycomponent(im, comps, clean_beam=cb) is im
    assert im.attrs["clean_beam"] == cb
    assert isinstance(im["pixels"].data, torch.Tensor) == on_device
    nchan, npol = g["out_pixels"].shape[:2]
    freq = np.asarray(im.frequency.data)
    flux = np.stack([_image_flux(c, freq, nchan, npol, True)
                     for c in (comps if isinstance(comps, list) else [comps])])
    _assert_restored(_np(im["pixels"].data), g["out_pixels"], flux, tag)


@pytest.mark.parametrize("what,sigma,extra", [("narrow beam, pruned", 0.8, []),
                                              ("wide beam, nothing pruned", 30.0, []),
                                              ("wide beam, component at (-40, -40)", 30.0,
                                               [(-40.0, -40.0)])])
def test_restore_lattice_against_unpruned_restatement(what, sigma, extra):
    from ska_sdp_func_python_amd.sky_component import restore_skycomponent
    rng = np.random.default_rng(14)
    geometry = R.geometry(3, "stokesIQUV")
    pos = np.array(list(R.lattice()) + extra)
    flux = rng.uniform(-5.0, 5.0, (len(pos), 3, 4))
    comps = R.components_at(R.make_image(geometry), pos, flux)
    cb = R.beam_of_sigma(sigma)
    got, ref = _both(lambda im: restore_skycomponent(im, comps, clean_beam=cb), geometry)
    _assert_restored(got, ref, flux, what)
    if extra:  # the component off the image has added its tail
        alone = R.restore(np.zeros_like(ref), [extra[0]], flux[-1:], 0.5 / sigma**2, 0.0, 0.5 / sigma**2)
        assert np.abs(alone).max() > 1e3 * RESTORE_TOL * np.abs(flux).sum(axis=0).max()


def test_restore_float32_pixels():
    from ska_sdp_func_python_amd.sky_component import restore_skycomponent
    g = R.load("restore_iquv")
    comps = R.make_components(g)
    got, ref = _both(lambda im: restore_skycomponent(im, comps, clean_beam=_beam(g)), g,
                     dtype=np.float32)
    # the pixel is rounded to float32 after every add; a term that differs in
    # its last fp64 bits may round to the neighbouring float32, so per
    # component at most one float32 ulp of the largest value a pixel can pass
    # through, max|start| + sum|flux| (the fluxes are the components' as is)
    largest = np.abs(R.start_pixels(3, 4)).max(axis=(2, 3)) + np.abs(g["comp_flux"]).sum(axis=0)
    bound = len(comps) * np.spacing(largest.astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=(2, 3))
    print(f"\n  restore float32: max error {err.max():.2e}, bound {bound.min():.2e}")
    assert np.all(err <= bound)


# ---- 6. Voronoi -------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [True, False])
def test_voronoi_labels_and_masks(on_device):
    from ska_sdp_func_python_amd.sky_component import image_voronoi_iter, voronoi_decomposition
    g = R.load("voronoi")
    im = R.make_image(g, to=_t if on_device else None)
    comps = R.make_components(g)
    vor, labels = voronoi_decomposition(im, comps)
    assert np.array_equal(vor.points, g["points"])
    assert isinstance(labels, torch.Tensor) == on_device
    if on_device:
        assert labels.is_cuda and labels.dtype == torch.int64
    assert _np(labels).dtype == g["labels"].dtype and np.array_equal(_np(labels), g["labels"])
    masks = list(image_voronoi_iter(im, comps))
    assert len(masks) == 9
    for region, m in enumerate(masks):
        data = m["pixels"].data
        assert isinstance(data, torch.Tensor) == on_device and tuple(data.shape) == (1, 1, R.NY, R.NX)
        if on_device:
            assert data.is_cuda and data.dtype == torch.float64
        assert np.array_equal(_np(data)[0, 0], (g["labels"] == region).astype(float))


@pytest.mark.parametrize("swap", [False, True])
def test_voronoi_exact_tie_takes_the_lower_index(swap):
    """Two points at exactly representable positions, mirror images about pixel
    column 21: every pixel of that column is equally far from both."""
    from ska_sdp_func_python_amd import kernels
    pair = [(20.25, 30.5), (21.75, 30.5)]
    xy = np.array([(3.5, 70.25)] + (pair[::-1] if swap else pair) + [(55.0, 5.0)])
    labels = kernels.skycomp_nearest(R.NY, R.NX, xy, _dev()).cpu().numpy()
    assert np.array_equal(labels, R.nearest(R.NY, R.NX, xy))
    column = labels[:, 21]
    assert np.all((column == 1) | (column == 0) | (column == 3)) and np.count_nonzero(column == 1) > 40
    assert not np.any(column == 2)
    # many components, more than one LDS chunk of them
    rng = np.random.default_rng(15)
    many = np.stack([rng.uniform(0, R.NX, 1500), rng.uniform(0, R.NY, 1500)], 1)
    got = kernels.skycomp_nearest(R.NY, R.NX, many, _dev()).cpu().numpy()
    assert np.array_equal(got, R.nearest(R.NY, R.NX, many))


# ---- 7. residency -----------------------------------------------------------------
def test_device_image_is_updated_in_its_own_storage():
    from ska_sdp_func_python_amd.sky_component import (image_voronoi_iter, insert_skycomponent,
                                                       restore_skycomponent)
    g = R.load("insert_lanczos")
    im = R.make_image(g, to=_t)
    data = im["pixels"].data
    ptr = data.data_ptr()
    comps = R.make_components(g)
    insert_skycomponent(im, comps, insert_method="Lanczos")
    restore_skycomponent(im, comps[:2], clean_beam=R.beam_of_sigma(2.0))
    assert im["pixels"].data is data and data.data_ptr() == ptr and data.is_cuda
    assert not np.array_equal(_np(data), R.start_pixels(3, 4))
    one = list(image_voronoi_iter(im, comps[:1]))
    assert len(one) == 1 and one[0]["pixels"].data.is_cuda and bool((one[0]["pixels"].data == 1).all())
    # numpy in, numpy out, the same array
    host = R.make_image(g)
    arr = host["pixels"].data
    insert_skycomponent(host, comps, insert_method="Lanczos")
    assert host["pixels"].data is arr and isinstance(arr, np.ndarray)
    assert np.array_equal(arr, g["out_pixels"])
    # no components: nothing is touched
    before = data.clone()
    insert_skycomponent(im, [])
    restore_skycomponent(im, [], clean_beam=R.beam_of_sigma(2.0))
    assert torch.equal(data, before)
