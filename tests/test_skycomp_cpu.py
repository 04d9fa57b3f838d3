"""CPU checks of the sky-component image operations: the numpy restatements
(tests/skycomp_restatement.py) against the reference's outputs in
tests/golden/skycomp_*.npz, the host tap tables against the reference's insert
functions, the Python layer of sky_component/operations.py with the three
kernel wrappers replaced by the restatements, and the per-tile component
lists that the wrappers hand to the kernels."""

import logging

import numpy as np
import pytest
import torch

import skycomp_restatement as R

INSERT_CASES = ["nearest", "sinc", "lanczos", "pswf", "lanczos_bw", "freq5", "nearest_off", "single"]
RESTORE_CASES = ["single", "iquv", "freq5"]


@pytest.fixture
def host_layer():
    with R.host_kernels():
        yield


def _insert(g, im=None, comps=None):
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    im = R.make_image(g) if im is None else im
    comps = R.make_components(g) if comps is None else comps
    return im, insert_skycomponent(im, comps, insert_method=str(g["method"]),
                                   bandwidth=float(g["bandwidth"]), support=int(g["support"]))


def _beam(g):
    return dict(zip(("bmaj", "bmin", "bpa"), (float(v) for v in g["clean_beam"])))


# ---- 1. restatements against the reference ----------------------------------
def _captured(monkeypatch, name):
    """Replace a kernel wrapper by one that only records its arguments."""
    from ska_sdp_func_python_amd import kernels
    calls = []
    monkeypatch.setattr(kernels, name, lambda image, *a: calls.append(a) or image)
    return calls


@pytest.mark.parametrize("tag", INSERT_CASES)
def test_insert_restatement_is_bit_equal(tag, host_layer, monkeypatch):
    g = R.load(f"insert_{tag}")
    calls = _captured(monkeypatch, "skycomp_insert")
    im, _ = _insert(g)
    assert len(calls) == 1 and np.array_equal(im["pixels"].data, R.start_pixels(*im["pixels"].shape))
    out = R.insert(R.start_pixels(*im["pixels"].shape), *calls[0])
    assert np.array_equal(out, g["out_pixels"])
    assert not np.array_equal(out, R.start_pixels(*im["pixels"].shape))


@pytest.mark.parametrize("tag", RESTORE_CASES)
def test_restore_restatement_is_bit_equal(tag, host_layer, monkeypatch):
    from ska_sdp_func_python_amd.sky_component import restore_skycomponent
    g = R.load(f"restore_{tag}")
    calls = _captured(monkeypatch, "skycomp_restore")
    im = R.make_image(g)
    restore_skycomponent(im, R.make_components(g), clean_beam=_beam(g))
    out = R.restore(R.start_pixels(*im["pixels"].shape), *calls[0])
    assert np.array_equal(out, g["out_pixels"])


def test_nearest_restatement_is_equal():
    g = R.load("voronoi")
    labels = R.nearest(R.NY, R.NX, g["points"])
    assert labels.dtype == g["labels"].dtype and np.array_equal(labels, g["labels"])
    assert np.array_equal(np.bincount(labels.ravel()), g["region_counts"])


# ---- 2. the tap tables --------------------------------------------------------
def test_insert_functions_are_the_references_bit_for_bit():
    from ska_sdp_func_python_amd.sky_component import operations as ops
    g = R.load("taps")
    assert np.array_equal(ops.insert_function_sinc(g["x"]), g["sinc"])
    assert np.array_equal(ops.insert_function_L(g["x"]), g["lanczos"])
    assert np.array_equal(ops.insert_function_pswf(g["x"]), g["pswf"])
    # the reference's sinc starts from zeros: 0 at 0, not 1
    assert ops.insert_function_sinc(np.array([0.0, -0.0]))[0] == 0.0
    assert g["pswf"][np.abs(g["x"]) > 5].max() == 0.0 and g["pswf"].max() > 0.0


# ---- 3. the Python layer with the kernels replaced ---------------------------
@pytest.mark.parametrize("tag", INSERT_CASES)
def test_insert_host_layer(tag, host_layer, caplog):
    g = R.load(f"insert_{tag}")
    with caplog.at_level(logging.WARNING, logger="func-python-logger"):
        im, ret = _insert(g)
    assert ret is im
    assert isinstance(im["pixels"].data, np.ndarray)
    assert np.array_equal(im["pixels"].data, g["out_pixels"])
    if tag == "nearest_off":
        assert f"{int(g['nbad'])} components of {len(g['comp_flux'])} do not fit" in caplog.text
    else:
        assert "do not fit" not in caplog.text


def test_insert_bare_component_equals_list(host_layer):
    g = R.load("insert_single")
    bare = R.make_components(g)
    im1, _ = _insert(g, comps=bare)
    im2, _ = _insert(g, comps=[bare])
    assert np.array_equal(im1["pixels"].data, im2["pixels"].data)
    assert np.array_equal(im1["pixels"].data, g["out_pixels"])


@pytest.mark.parametrize("tag", RESTORE_CASES)
def test_restore_host_layer(tag, host_layer):
    from ska_sdp_func_python_amd.sky_component import restore_skycomponent
    g = R.load(f"restore_{tag}")
    im = R.make_image(g)
    assert im.attrs["clean_beam"] is None
    cb = _beam(g)
    comps = R.make_components(g)
    assert restore_skycomponent(im, comps, clean_beam=cb) is im
    assert im.attrs["clean_beam"] == cb
    assert np.array_equal(im["pixels"].data, g["out_pixels"])
    if int(g["single"]):
        im2 = R.make_image(g)
        restore_skycomponent(im2, [comps], clean_beam=cb)
        assert np.array_equal(im2["pixels"].data, g["out_pixels"])


def test_non_point_shape_raises_and_changes_nothing(host_layer):
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent, restore_skycomponent
    g = R.load("insert_lanczos")
    comps = R.make_components(g)
    comps[5].shape = "Gaussian"
    for call in (lambda im: insert_skycomponent(im, comps, insert_method="Lanczos"),
                 lambda im: insert_skycomponent(im, comps),
                 lambda im: restore_skycomponent(im, comps, clean_beam=R.beam_of_sigma(2.0))):
        im = R.make_image(g)
        with pytest.raises(ValueError, match="Cannot handle shape Gaussian"):
            call(im)
        assert np.array_equal(im["pixels"].data, R.start_pixels(3, 4))


@pytest.mark.parametrize("x,y", [(7.3, 40.6), (53.7, 40.6), (30.4, 7.3), (30.4, 75.7)])
@pytest.mark.parametrize("method", ["Sinc", "Lanczos", "PSWF"])
def test_window_one_pixel_over_a_border_raises_and_changes_nothing(host_layer, method, x, y):
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    im = R.make_image(R.geometry(3, "stokesIQUV"))
    flux = np.ones((2, 1, 4))
    # the first component fits: it must not have been inserted when the second fails
    comps = R.components_at(im, [(30.4, 40.6), (x, y)], flux, frequency=[1.0e8])
    with pytest.raises(ValueError, match="does not fit on the image"):
        insert_skycomponent(im, comps, insert_method=method)
    assert np.array_equal(im["pixels"].data, R.start_pixels(3, 4))
    # one pixel further in, the window is flush with the border
    inward = (x + (1 if x < 10 else -1 if x > 50 else 0), y + (1 if y < 10 else -1 if y > 70 else 0))
    insert_skycomponent(im, R.components_at(im, [inward], flux, frequency=[1.0e8]), insert_method=method)
    assert not np.array_equal(im["pixels"].data, R.start_pixels(3, 4))


@pytest.mark.parametrize("method", ["Nearest", "Lanczos"])
def test_single_channel_flux_is_broadcast(host_layer, method):
    from ska_sdp_func_python_amd import kernels
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent
    im = R.make_image(R.geometry(3, "stokesIQUV"))
    flux = np.array([[[2.0, 0.5, -0.25, 0.125]]])
    seen = []
    inner = kernels.skycomp_insert
    kernels.skycomp_insert = lambda image, *a: seen.append(a[-1]) or inner(image, *a)
    insert_skycomponent(im, R.components_at(im, [(30.4, 40.6)], flux, frequency=[1.0e8]),
                        insert_method=method)
    assert seen[0].shape == (1, 3, 4) and np.array_equal(seen[0][0], np.repeat(flux[0], 3, axis=0))
    added = im["pixels"].data - R.start_pixels(3, 4)
    assert all(np.abs(added[chan]).max() > 0 for chan in range(3))
    if method == "Nearest":  # the starting pixels and the flux are eighths: exact
        for chan in range(3):
            assert np.array_equal(added[chan, :, 41, 30], flux[0, 0])
        assert np.count_nonzero(added) == 12


def test_no_components_leave_the_image_untouched(host_layer):
    from ska_sdp_func_python_amd.sky_component import insert_skycomponent, restore_skycomponent
    im = R.make_image(R.geometry(3, "stokesIQUV"))
    assert insert_skycomponent(im, [], insert_method="Lanczos") is im
    assert insert_skycomponent(im, []) is im
    cb = R.beam_of_sigma(2.0)
    assert restore_skycomponent(im, [], clean_beam=cb) is im
    assert im.attrs["clean_beam"] == cb
    assert np.array_equal(im["pixels"].data, R.start_pixels(3, 4))


def test_voronoi_host_layer(host_layer):
    from ska_sdp_func_python_amd.sky_component import image_voronoi_iter, voronoi_decomposition
    g = R.load("voronoi")
    im = R.make_image(g)
    comps = R.make_components(g)
    vor, labels = voronoi_decomposition(im, comps)
    assert np.array_equal(vor.points, g["points"])
    assert isinstance(labels, np.ndarray) and labels.dtype == g["labels"].dtype
    assert np.array_equal(labels, g["labels"])
    masks = list(image_voronoi_iter(im, comps))
    assert len(masks) == 9
    for region, m in enumerate(masks):
        data = m["pixels"].data
        assert data.shape == (1, 1, R.NY, R.NX) and data.dtype == np.float64
        assert np.array_equal(data[0, 0], (g["labels"] == region).astype(float))
        assert int(data.sum()) == g["region_counts"][region]


def test_voronoi_iter_with_one_component_is_all_ones(host_layer):
    from ska_sdp_func_python_amd.sky_component import image_voronoi_iter
    g = R.load("voronoi")
    im = R.make_image(R.geometry(3, "stokesIQUV"))
    masks = list(image_voronoi_iter(im, R.make_components(g)[:1]))
    assert len(masks) == 1
    data = masks[0]["pixels"].data
    assert data.shape == (3, 4, R.NY, R.NX) and np.all(data == 1.0)
    assert masks[0].image_acc.polarisation_frame == im.image_acc.polarisation_frame


# ---- 4. the per-tile component lists ------------------------------------------
def _lists(boxes, start, stop, ny, nx):
    from ska_sdp_func_python_amd import kernels
    ptr, comp = (t.numpy() for t in kernels.tile_csr(boxes, start, stop, ny, nx, torch.device("cpu")))
    assert ptr.dtype == np.int64 and comp.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(comp)
    return [comp[ptr[t]:ptr[t + 1]] for t in range(len(ptr) - 1)]


def test_tile_lists_hold_every_overlapping_component_in_order():
    from ska_sdp_func_python_amd import _lib, kernels
    tx, ty = _lib.SDP_HIP_SKYCOMP_TILE_X, _lib.SDP_HIP_SKYCOMP_TILE_Y
    rng = np.random.default_rng(5)
    ny, nx, n = R.NY, R.NX, 200
    x_lo, y_lo = rng.integers(-40, nx + 20, n), rng.integers(-40, ny + 20, n)
    x_hi, y_hi = x_lo + rng.integers(0, 40, n), y_lo + rng.integers(0, 40, n)
    boxes = kernels.tile_boxes(x_lo, x_hi, y_lo, y_hi, ny, nx)
    lists = _lists(boxes, 0, n, ny, nx)
    tiles_x = -(-nx // tx)
    assert len(lists) == tiles_x * -(-ny // ty)
    for t, comps in enumerate(lists):
        px0, py0 = (t % tiles_x) * tx, (t // tiles_x) * ty
        px1, py1 = min(px0 + tx, nx) - 1, min(py0 + ty, ny) - 1
        want = np.flatnonzero((x_lo <= px1) & (x_hi >= px0) & (y_lo <= py1) & (y_hi >= py0))
        assert np.array_equal(comps, want), t
    assert sum(len(c) for c in lists) == boxes[3].sum()


def test_launches_split_the_components_in_order(monkeypatch):
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(6)
    n = 50
    x_lo, y_lo = rng.integers(0, R.NX, n), rng.integers(0, R.NY, n)
    boxes = kernels.tile_boxes(x_lo, x_lo + 20, y_lo, y_lo + 20, R.NY, R.NX)
    monkeypatch.setattr(kernels.skycomp, "SKYCOMP_MAX_PAIRS", 25)
    ranges = list(kernels.skycomp._skycomp_launches(boxes, n))
    assert len(ranges) > 3 and ranges[0][0] == 0 and ranges[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    for s, e in ranges:
        assert e > s and (boxes[3][s:e].sum() <= 25 or e == s + 1)
    whole = _lists(boxes, 0, n, R.NY, R.NX)
    parts = [_lists(boxes, s, e, R.NY, R.NX) for s, e in ranges]
    for t, comps in enumerate(whole):
        joined = np.concatenate([p[t] + s for p, (s, _) in zip(parts, ranges)])
        assert np.array_equal(joined, comps)


def test_restore_leaves_out_only_what_underflows(monkeypatch):
    """Every (tile, component) pair that the restore wrapper does not list has
    an exponent argument above 700 on the whole tile."""
    from ska_sdp_func_python_amd import _lib, kernels
    from ska_sdp_func_python_amd.image.deconvolution import _gaussian_coefficients
    tx, ty = _lib.SDP_HIP_SKYCOMP_TILE_X, _lib.SDP_HIP_SKYCOMP_TILE_Y
    a, b, c = _gaussian_coefficients(0.5, 1.1, np.deg2rad(-60.0))
    xy = np.array([(20.3, 30.7), (-10.4, 40.3), (60.2, 82.9), (-200.0, 30.0)])
    seen = {}
    monkeypatch.setattr(kernels.skycomp, "_skycomp_image", lambda image: (1, R.NY, R.NX))
    monkeypatch.setattr(kernels.skycomp, "ptr", lambda v: v)
    monkeypatch.setattr(kernels.skycomp, "stream", lambda dev: None)
    monkeypatch.setattr(_lib, "call", lambda name, *args: seen.update(ptr=args[11].numpy(),
                                                                     comp=args[12].numpy()))
    image = torch.zeros((1, 1, R.NY, R.NX), dtype=torch.float64)
    kernels.skycomp_restore(image, xy, np.ones((4, 1, 1)), a, b, c)
    ptr, comp = seen["ptr"], seen["comp"]
    tiles_x = -(-R.NX // tx)
    row, col = np.indices((R.NY, R.NX))
    listed = pruned = 0
    for t in range(len(ptr) - 1):
        sl = (slice((t // tiles_x) * ty, (t // tiles_x + 1) * ty), slice((t % tiles_x) * tx, (t % tiles_x + 1) * tx))
        for k in range(len(xy)):
            dx, dy = col[sl] - xy[k, 0], row[sl] - xy[k, 1]
            arg = a * dx**2 + b * dx * dy + c * dy**2
            if k in comp[ptr[t]:ptr[t + 1]]:
                listed += 1
            else:
                pruned += 1
                assert arg.min() > 700.0, (t, k)
            if arg.min() < 600.0:
                assert k in comp[ptr[t]:ptr[t + 1]]
    assert listed > 0 and pruned > 0
