"""Batched Gaussian fits on the device (csrc/gaussfit.hip) against the host
restatement of tests/gaussfit_restatement.py, and fit_skycomponent and
find_skycomponents_frequency_taylor_terms end to end.

The restatement is written from numpy and scipy.optimize.leastsq, the MINPACK
solver that the reference runs through astropy's LevMarLSQFitter; it is not a
run of the reference, whose astropy is not available where this project is
built (the restatement's docstring says which lines of the reference and which
behaviour of astropy 5.2 each step restates).

Tolerance: measured, not chosen.  S (tests/golden/gaussfit_windows.npz, written
by tests/golden/make_golden_gaussfit.py) is per parameter the largest
difference between the yardstick at the reference's stop (xtol 1e-7, ftol
1.49e-8) and at xtol = ftol = 1e-14 over the committed cases.  The device's
parameters must lie within 2 S of the tight yardstick: as loosely converged as
the reference's own answer, on either side, and no looser.  theta is compared
for sources with an axial ratio of at least 1.3 only.  Every case keeps its
centre 0.05 pixel from a half-integer, so the pixel that the centre rounds to,
and with it the flux, must be EQUAL to the yardstick's.
"""

import numpy as np
import pytest

import gaussfit_restatement as gr
import skycomp_restatement as sr

pytestmark = pytest.mark.gpu

NAMES = list(gr.WINDOW_CASES)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device: the gpu tests need an MI355X")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return gr.load("windows")


def on(dev, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def fit(planes, x0, y0, **kw):
    from ska_sdp_func_python_amd import kernels
    params, status, niter = kernels.gauss_fit(planes, x0, y0, **kw)
    assert str(params.dtype) == "torch.float64" and params.is_cuda
    assert tuple(params.shape) == (len(planes), 6)
    assert str(status.dtype) == "torch.int32" and str(niter.dtype) == "torch.int32"
    return params, status, niter


def compare(S, got, want, label=""):
    """Device parameters against the tight yardstick's: within 2 S, theta for
    elongated sources only, and the same rounded pixel."""
    got, want = np.asarray(got), np.asarray(want)
    diff = np.abs(got - want)
    n = 6 if gr.axial_ratio(want) >= gr.THETA_AXIAL_RATIO else 5
    print(f"{label}: |device - tight| / S =", np.array2string(diff[:n] / S[:n], precision=3))
    assert np.all(diff[:n] <= 2.0 * S[:n]), (label, diff, 2.0 * S)
    assert (round(got[1]), round(got[2])) == (round(want[1]), round(want[2])), label


def yardstick(plane, x0, y0):
    """The tight yardstick on a host plane, with the conditions on a case."""
    t = gr.fit_plane(np.asarray(plane, dtype=np.float64), x0, y0, tight=True)
    assert t["converged"] and gr.half_pixel_margin(t["params"]) >= gr.HALF_PIXEL_MARGIN
    return t["params"]


# ---- the committed cases ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def home(dev):
    """Per dtype: the host planes of every case at its home, their device
    copies, the origins, and the results of one batch over all of them."""
    out = {}
    for dtype in (np.float64, np.float32):
        host = [gr.home_plane(name, dtype) for name in NAMES]
        planes = [on(dev, p) for p in host]
        x0 = [gr.WINDOW_HOMES[name][0] for name in NAMES]
        y0 = [gr.WINDOW_HOMES[name][1] for name in NAMES]
        params, status, niter = fit(planes, x0, y0)
        out[dtype] = dict(host=host, planes=planes, x0=x0, y0=y0, params=params, status=status,
                          niter=niter)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_float64_cases_against_the_fixture(home, golden, name):
    """Noiseless and noisy, circular and rotated either way, offsets on both
    sides of the centre pixel, negative amplitude; planes of different sizes
    in one batch, homes up to pixel 4000."""
    k = NAMES.index(name)
    h = home[np.float64]
    assert len({p.shape for p in h["planes"]}) > 10
    assert int(h["status"][k]) == 0 and 1 < int(h["niter"][k]) <= 100
    compare(golden["S"], h["params"][k].cpu().numpy(), golden["tight"][k], name)
    # the planes are only read
    assert np.array_equal(h["planes"][k].cpu().numpy(), h["host"][k])


@pytest.mark.parametrize("name", NAMES)
def test_float32_cases_against_the_yardstick(home, golden, name):
    k = NAMES.index(name)
    h = home[np.float32]
    assert h["planes"][k].dtype.itemsize == 4 and int(h["status"][k]) == 0
    want = yardstick(h["host"][k], h["x0"][k], h["y0"][k])
    compare(golden["S"], h["params"][k].cpu().numpy(), want, name)
    assert np.array_equal(h["planes"][k].cpu().numpy(), h["host"][k])


# ---- batches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfit", [1, 4, 5, 257])
def test_batch_equals_single_fits_bit_for_bit(home, nfit):
    """257 fits cross a block (4 fits) and leave the last block one wave."""
    import torch
    h = home[np.float64]
    pick = [(3 * n + 1) % len(NAMES) for n in range(nfit)]
    args = ([h["planes"][k] for k in pick], [h["x0"][k] for k in pick], [h["y0"][k] for k in pick])
    params, status, niter = fit(*args)
    again = fit(*args)
    assert torch.equal(bits(params), bits(again[0])) and torch.equal(status, again[1])
    assert torch.equal(niter, again[2])
    for n, k in enumerate(pick):
        if n >= len(NAMES):
            # a repeat of an earlier entry of the batch
            assert torch.equal(bits(params[n]), bits(params[n - len(NAMES)]))
            continue
        alone = fit([h["planes"][k]], [h["x0"][k]], [h["y0"][k]])
        assert torch.equal(bits(alone[0][0]), bits(params[n])), NAMES[k]
        assert torch.equal(bits(alone[0][0]), bits(h["params"][k]))
        assert int(alone[1][0]) == int(status[n]) == 0 and int(alone[2][0]) == int(niter[n])


# ---- geometry -----------------------------------------------------------------------------------------
def test_geometry(dev, golden):
    """The whole plane as the window; 16 x 17; windows flush with each border;
    views whose row stride exceeds their width; all in one batch."""
    S = golden["S"]
    w = {name: gr.case_window(name) for name in ("ellipse_pos_noisy", "beam_noisy",
                                                  "ellipse_neg_noisy", "wide")}
    jobs = []   # (label, device plane, host plane, x0, y0)

    def add(label, host, x0, y0, view=None):
        t = on(dev, host) if view is None else view
        jobs.append((label, t, host, x0, y0))

    add("15x15", w["ellipse_pos_noisy"].copy(), 0, 0)
    for x0, y0 in ((0, 0), (2, 1), (2, 0), (0, 1)):
        add(f"16x17 at {x0},{y0}", gr.placed((16, 17), w["beam_noisy"], x0, y0), x0, y0)
    ny, nx = 40, 50
    for x0, y0 in ((0, 11), (nx - 15, 13), (17, 0), (19, ny - 15), (nx - 15, ny - 15)):
        add(f"40x50 at {x0},{y0}", gr.placed((ny, nx), w["ellipse_neg_noisy"], x0, y0), x0, y0)
    # a channel and polarisation of a cube: the view starts inside the allocation
    cube = 1e-3 * np.random.default_rng(2).standard_normal((3, 2, ny, nx))
    cube[1, 1, 9:24, 30:45] = w["wide"]
    dcube = on(dev, cube)
    add("cube[1, 1]", cube[1, 1], 30, 9, view=dcube[1, 1])
    # a column block of a wider image: row stride 60, width 30
    wide = gr.placed((25, 60), w["ellipse_pos_noisy"], 20, 10)
    dwide = on(dev, wide)
    view = dwide[:, 12:42]
    assert view.stride(0) == 60 and view.shape[1] == 30
    add("columns 12:42", wide[:, 12:42], 8, 10, view=view)
    # rows from 3 on, float64 view of the same image
    add("rows 3:", wide[3:], 20, 7, view=dwide[3:])
    params, status, _ = fit([j[1] for j in jobs], [j[3] for j in jobs], [j[4] for j in jobs])
    params = params.cpu().numpy()
    assert not status.any().item()
    for n, (label, t, host, x0, y0) in enumerate(jobs):
        compare(S, params[n], yardstick(host, x0, y0), label)
        assert np.array_equal(t.cpu().numpy(), host)
    assert np.array_equal(dcube.cpu().numpy(), cube) and np.array_equal(dwide.cpu().numpy(), wide)


# ---- what is not finite, and what is refused ----------------------------------------------------------
def test_nan_window_is_status_2_and_leaves_its_neighbours(home, dev):
    import torch
    h = home[np.float64]
    pick = [0, 3, 7, 9, 12]
    planes = [h["planes"][k] for k in pick]
    x0, y0 = [h["x0"][k] for k in pick], [h["y0"][k] for k in pick]
    clean = fit(planes, x0, y0)
    for bad, corner in ((np.nan, (0, 0)), (np.inf, (14, 14)), (-np.inf, (7, 3))):
        host = h["host"][pick[2]].copy()
        host[y0[2] + corner[0], x0[2] + corner[1]] = bad
        dirty = list(planes)
        dirty[2] = on(dev, host)
        params, status, niter = fit(dirty, x0, y0)
        assert status.tolist() == [0, 0, 2, 0, 0]
        assert torch.isnan(params[2]).all().item()
        keep = [0, 1, 3, 4]
        assert torch.equal(bits(params[keep]), bits(clean[0][keep]))
        assert torch.equal(niter[keep], clean[2][keep])
    # a NaN outside the window is not read
    host = h["host"][pick[0]].copy()
    outside = np.ones(host.shape, dtype=bool)
    outside[y0[0]:y0[0] + 15, x0[0]:x0[0] + 15] = False
    host[outside] = np.nan
    params, status, _ = fit([on(dev, host)], x0[:1], y0[:1])
    assert int(status[0]) == 0 and torch.equal(bits(params[0]), bits(clean[0][0]))


def test_max_iter_and_refusals(home, dev):
    import torch
    from ska_sdp_func_python_amd import kernels
    h = home[np.float64]
    k = NAMES.index("ellipse_neg_noisy")
    one = ([h["planes"][k]], [h["x0"][k]], [h["y0"][k]])
    params, status, niter = fit(*one, max_iter=3)
    assert int(status[0]) == 1 and int(niter[0]) == 3 and torch.isfinite(params).all().item()
    empty = fit([], [], [])
    assert empty[0].shape == (0, 6) and empty[1].shape == (0,)
    plane = h["planes"][k]
    ny, nx = plane.shape
    for x0, y0 in ((-1, 0), (0, -1), (nx - 14, 0), (0, ny - 14)):
        with pytest.raises(ValueError, match="does not lie on its plane"):
            kernels.gauss_fit([plane], [x0], [y0])
    with pytest.raises(ValueError, match="agree in dtype"):
        kernels.gauss_fit([plane, home[np.float32]["planes"][k]], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="x stride"):
        kernels.gauss_fit([torch.zeros((40, 40), dtype=torch.float64, device=dev).t()], [0], [0])
    with pytest.raises(ValueError, match="device"):
        kernels.gauss_fit([torch.zeros((40, 40), dtype=torch.float64)], [0], [0])
    with pytest.raises(ValueError, match="float32 or float64"):
        kernels.gauss_fit([torch.zeros((40, 40), dtype=torch.int32, device=dev)], [0], [0])
    with pytest.raises(ValueError, match="max_iter"):
        kernels.gauss_fit([plane], [0], [0], max_iter=0)
    with pytest.raises(ValueError, match="planes"):
        kernels.gauss_fit([plane], [0, 1], [0])


# ---- fit_skycomponent end to end ------------------------------------------------------------------------
def _restored(to):
    """A 64 x 96 IQUV image of 3 channels with six components restored with an
    elliptical beam: at x = 7 and y = ny - 8, and at x = nx - 8 and y = 7, the
    windows are flush with two borders each; at x = 6, x = nx - 7, y = 6 and
    y = ny - 7 they leave the image by one pixel."""
    from ska_sdp_func_python_amd.sky_component import operations as ops
    ny, nx = 64, 96
    g = sr.geometry(3, "stokesIQUV")
    g["shape"] = np.array([ny, nx])
    im = sr.make_image(g, pixels=np.zeros((3, 4, ny, nx)), to=to)
    positions = [(7, ny - 8), (nx - 8, 7), (6, 25), (nx - 7, 40), (40, 6), (60, ny - 7)]
    rng = np.random.default_rng(4)
    flux = rng.uniform(1.0, 3.0, (6, 3, 4))
    flux[:, :, 1:] *= 0.2
    comps = sr.components_at(im, positions, flux)
    fwhm = np.sqrt(8.0 * np.log(2.0)) * 0.001
    ops.restore_skycomponent(im, comps, clean_beam={"bmaj": 2.0 * fwhm, "bmin": 1.3 * fwhm,
                                                    "bpa": 25.0})
    return g, im, comps, [True, True, False, False, False, False]


def test_fit_skycomponent_end_to_end(dev, golden):
    import torch
    from ska_sdp_func_python_amd.sky_component import operations as ops
    S = golden["S"]
    g, im, comps, fitted = _restored(lambda p: on(dev, p))
    pixels = im["pixels"].data
    before = pixels.clone()
    got = [ops.fit_skycomponent(im, sc) for sc in comps]
    gauss = [ops.fit_skycomponent(im, sc, force_point_sources=False) for sc in comps]
    batch = ops.fit_skycomponents(im, comps)
    assert im["pixels"].data is pixels and pixels.is_cuda and torch.equal(pixels, before)
    host = pixels.cpu().numpy()
    him = sr.make_image(g, pixels=host.copy())
    again = [ops.fit_skycomponent(him, sc) for sc in comps]
    assert isinstance(him["pixels"].data, np.ndarray) and np.array_equal(him["pixels"].data, host)
    cell = np.deg2rad(g["cell_deg"])
    tol = 2.0 * cell * np.hypot(S[1], S[2]) + 1e-15
    scale = 2.0 * np.sqrt(2.0 * np.log(2.0)) * g["cell_deg"] * (host.shape[3] - 1) / host.shape[3]
    for k, sc in enumerate(comps):
        want = gr.fit_component(him, sc, tight=True, force_point_sources=False)
        assert want["fitted"] == fitted[k]
        if not fitted[k]:
            assert got[k] is sc and gauss[k] is sc and batch[0][k] is sc and again[k] is sc
            continue
        assert gr.half_pixel_margin(want["fit"]) >= gr.HALF_PIXEL_MARGIN
        new = got[k]
        assert new is not sc and new.shape == "Point" and new.name == sc.name
        assert isinstance(new.flux, np.ndarray) and new.flux.shape == (3, 4)
        assert np.array_equal(new.flux, want["flux"])
        assert np.array_equal(new.flux, host[:, :, round(want["fit"][2]), round(want["fit"][1])])
        sep = gr.angle_between(new.direction.ra.rad, new.direction.dec.rad, want["ra"], want["dec"])
        print(f"component {k}: separation {sep:.3e} rad, allowed {tol:.3e}")
        assert sep <= tol
        # the Gaussian params: widths within 2 S, theta (axial ratio 1.5) within 2 S
        assert gr.axial_ratio(want["fit"]) >= gr.THETA_AXIAL_RATIO
        gp, wp = gauss[k].params, want["params"]
        assert gauss[k].shape == "Gaussian" and np.array_equal(gauss[k].flux, new.flux)
        assert abs(gp["bmaj"] - wp["bmaj"]) <= np.rad2deg(2.0 * max(S[3], S[4]) * scale)
        assert abs(gp["bmin"] - wp["bmin"]) <= np.rad2deg(2.0 * max(S[3], S[4]) * scale)
        assert abs(gp["bpa"] - wp["bpa"]) <= np.rad2deg(2.0 * S[5])
        assert gp["bmaj"] > gp["bmin"] > 0
        # the batch and numpy pixels give the same component
        for other in (batch[0][k], again[k]):
            assert other.direction == new.direction and np.array_equal(other.flux, new.flux)
            assert other.shape == "Point"


# ---- find_skycomponents_frequency_taylor_terms ------------------------------------------------------------
@pytest.mark.parametrize("nmoment", [1, 3])
def test_find_skycomponents_frequency_taylor_terms(dev, nmoment):
    from ska_sdp_func_python_amd.sky_component import taylor_terms as tt
    images, threshold = gr.taylor_images(to=lambda p: on(dev, p))
    host_images, _ = gr.taylor_images()
    want = gr.find_taylor_terms(host_images, nmoment=nmoment, component_threshold=threshold)
    got = tt.find_skycomponents_frequency_taylor_terms(images, nmoment=nmoment,
                                                       component_threshold=threshold)
    assert all(im["pixels"].data.is_cuda for im in images)
    assert len(got) == len(want) == 5
    for chan, (gc, wc) in enumerate(zip(got, want)):
        assert len(gc) == len(wc) == 6
        assert [c.name for c in gc] == [c.name for c in wc] == [f"Segment {k}" for k in range(6)]
        for a, b in zip(gc, wc):
            assert a.flux.shape == (1, 2) and np.array_equal(a.flux, b.flux)
            assert np.array_equal(a.frequency, b.frequency)
            assert abs(a.direction.ra.rad - b.direction.ra.rad) <= 1e-12
            assert abs(a.direction.dec.rad - b.direction.dec.rad) <= 1e-12
    assert tt.find_skycomponents_frequency_taylor_terms(images, nmoment=nmoment,
                                                        component_threshold=10.0) == []
