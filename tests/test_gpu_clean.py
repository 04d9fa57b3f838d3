"""GPU parity of the CLEAN stage (csrc/clean.hip through image.cleaners and
image.deconvolution) against the reference's goldens and the numpy
restatement (tests/clean_restatement.py), and of restore_cube / fit_psf.

Tolerances
  Hogbom: 1e-12 * max|dirty| on components and residual, the project's bound
  where only fp64 rounding may differ (tests/test_gpu_weighting.py); with
  contraction off in clean.hip the match is expected to be exact.
  msclean: the minor cycle is the same arithmetic, the only extra difference
  is the set-up FFT (numpy.fft on the host for numpy input, torch.fft for
  device input).  Measured on the CPU, the restatement run with numpy.fft
  against the same run with torch.fft differs on M1, M1w, M2, M3, M4 by at
  most 7.1e-16 (M2's residual; components 2.8e-16 at most); 10x that is allowed.
"""

import functools

import numpy as np
import pytest
import torch

import clean_restatement as cr
from test_clean_cpu import HOGBOM, MSCLEAN, _image, load_case
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd import image, kernels
from ska_sdp_func_python_amd.image import cleaners

pytestmark = pytest.mark.gpu
MSCLEAN_FFT_DIFF = 7.1e-16  # see the module docstring
MSCLEAN_TOL = 10 * MSCLEAN_FFT_DIFF


def T(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=float), device="cuda:0")


def H(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


@functools.lru_cache(maxsize=None)
def restated(name):
    """(comps, residual, iterations) of the restatement, computed once per case."""
    c = load_case(name)
    if c["scales"]:
        out = cr.msclean(c["dirty"], c["psf"], c["window"], c["sens"], c["gain"], c["thresh"],
                         c["niter"], c["scales"], c["fracthresh"])
    else:
        out = cr.hogbom(c["dirty"], c["psf"], c["window"], c["gain"], c["thresh"], c["niter"],
                        c["fracthresh"])
    for a in out[:2]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", HOGBOM)
def test_hogbom_golden(name, on_device):
    c = load_case(name)
    conv = T if on_device else (lambda a: a)
    comps, res, info = cleaners.hogbom_run(conv(c["dirty"]), conv(c["psf"]), conv(c["window"]),
                                           c["gain"], c["thresh"], c["niter"], c["fracthresh"])
    assert isinstance(comps, torch.Tensor) == on_device and isinstance(res, torch.Tensor) == on_device
    comps, res = H(comps), H(res)
    tol = 1e-12 * np.abs(c["dirty"]).max()
    print(name, "comps", np.abs(comps - c["comps"]).max(), "res", np.abs(res - c["residual"]).max(),
          info)
    assert np.array_equal(comps != 0, c["comps"] != 0)
    assert np.abs(comps - c["comps"]).max() <= tol
    assert np.abs(res - c["residual"]).max() <= tol
    assert info["niter"] == restated(name)[2]
    plain = cleaners.hogbom(conv(c["dirty"]), conv(c["psf"]), conv(c["window"]), c["gain"],
                            c["thresh"], c["niter"], c["fracthresh"])
    assert len(plain) == 2 and np.array_equal(H(plain[0]), comps) and np.array_equal(H(plain[1]), res)


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", MSCLEAN)
def test_msclean_golden(name, on_device):
    c = load_case(name)
    conv = T if on_device else (lambda a: a)
    comps, res, info = cleaners.msclean_run(conv(c["dirty"]), conv(c["psf"]), conv(c["window"]),
                                            conv(c["sens"]), c["gain"], c["thresh"], c["niter"],
                                            c["scales"], c["fracthresh"])
    assert isinstance(comps, torch.Tensor) == on_device and isinstance(res, torch.Tensor) == on_device
    comps, res = H(comps), H(res)
    print(name, "comps", np.abs(comps - c["comps"]).max(), "res", np.abs(res - c["residual"]).max(),
          info)
    assert np.array_equal(comps != 0, c["comps"] != 0)
    assert np.abs(comps - c["comps"]).max() <= MSCLEAN_TOL
    assert np.abs(res - c["residual"]).max() <= MSCLEAN_TOL
    assert info["niter"] == restated(name)[2]


def test_msclean_odd_psf_keeps_the_scale_kernel_centre():
    """An odd PSF: the scale kernels sit at ceil(n / 2), one pixel off the PSF
    origin n // 2.  numpy input, so the set-up is the restatement's and the
    minor cycles must agree bit for bit."""
    inp = load_case("H3")
    want = cr.msclean(inp["dirty"], inp["psf"], None, None, 0.7, 0.0, 25, [0, 3, 6], 0.05)
    comps, res, info = cleaners.msclean_run(inp["dirty"], inp["psf"], None, None, 0.7, 0.0, 25,
                                            [0, 3, 6], 0.05)
    assert np.array_equal(comps, want[0]) and np.array_equal(res, want[1])
    assert info["niter"] == want[2]


def _tie_case():
    dirty = np.zeros((70, 70))
    dirty[3, 66] = dirty[40, 5] = 1.0
    psf = np.zeros((16, 16))
    psf[8, 8] = 1.0
    return dirty, psf


def test_exact_tie_takes_the_first_index_across_tiles():
    """Two equal peaks in different tiles: components and residual equal the
    restatement's bit for bit, so the lower flat index wins every tie.  After
    an even number of cycles both peaks have had the same share, so niter = 5
    is run as well: there the first peak is one component ahead."""
    dirty, psf = _tie_case()
    for niter in (6, 5):
        want = cr.hogbom(dirty, psf, None, 0.5, 0.0, niter, 0.0)
        assert want[0][3, 66] != 0 and want[0][40, 5] != 0
        assert (want[0][3, 66] > want[0][40, 5]) == (niter == 5)
        for conv in (lambda a: a, T):
            comps, res, info = cleaners.hogbom_run(conv(dirty), conv(psf), None, 0.5, 0.0, niter, 0.0)
            assert np.array_equal(H(comps), want[0]) and np.array_equal(H(res), want[1])
            assert info["niter"] == want[2] == niter


def test_exact_tie_across_scales_takes_the_lower_scale():
    """The same pair in an S = 2 msclean with scales [0, 0] (two identical
    scale planes): bit-equal to the restatement."""
    dirty, psf = _tie_case()
    want = cr.msclean(dirty, psf, None, None, 0.5, 0.0, 6, [0, 0], 0.0)
    comps, res, info = cleaners.msclean_run(dirty, psf, None, None, 0.5, 0.0, 6, [0, 0], 0.0)
    assert np.array_equal(comps, want[0]) and np.array_equal(res, want[1])
    assert info["niter"] == want[2]


def test_scale_tie_is_visible_in_the_components():
    """Two bit-identical residual planes whose scale kernels differ: the
    component written shows that the lower scale and the first pixel won."""
    dirty, psf = _tie_case()
    res = T(np.stack([dirty, dirty]))
    delta = np.zeros((2, 2, 16, 16))
    delta[:, :, 8, 8] = 1.0
    skern = np.zeros((2, 16, 16))
    skern[0, 8, 8], skern[1, 8, 8] = 1.0, 3.0
    comps = torch.zeros(70, 70, dtype=torch.float64, device="cuda:0")
    done, stop = kernels.clean_plane("msclean", res, T(delta), comps, 0.5, 1.0, 0.0, 1,
                                     coupling_diag=[1.0, 1.0], scale_kernels=T(skern))
    assert (done, stop) == (1, "niter")
    expect = np.zeros((70, 70))
    expect[3, 66] = 0.5
    assert np.array_equal(H(comps), expect)
    assert np.array_equal(H(res)[0], dirty - expect) and np.array_equal(H(res)[1], dirty - expect)


# ---- deconvolve_cube -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cube():
    """[2 chan, 4 pol] 64 x 48 dirty cube and PSF cube (pol 2's PSF is zero)."""
    rng = np.random.default_rng(11)
    uv = rng.normal(0.0, 0.12, (200, 2))
    y, x = np.mgrid[0:64, 0:48]

    def beam(dy, dx):
        return np.cos(2 * np.pi * (uv[:, 0, None, None] * dx + uv[:, 1, None, None] * dy)).mean(0)

    psf = np.zeros((2, 4, 64, 48))
    psf[:] = beam(y - 32, x - 24)
    psf[:, 2] = 0.0
    dirty = rng.normal(0.0, 0.02, (2, 4, 64, 48))
    for chan in range(2):
        for pol in range(4):
            for _ in range(5):
                py, px = rng.integers(8, 56), rng.integers(8, 40)
                dirty[chan, pol] += rng.uniform(0.3, 1.0) * beam(y - py, x - px)
    dirty.setflags(write=False)
    psf.setflags(write=False)
    return dirty, psf


def _cube_images(on_device=False):
    dirty, psf = _cube()
    conv = T if on_device else np.array
    return _image(conv(dirty)), _image(conv(psf))


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
def test_deconvolve_cube_planes_and_zero_psf_pol(on_device):
    dirty, psf = _cube()
    comp, resid = image.deconvolve_cube(*_cube_images(on_device), algorithm="hogbom", niter=40,
                                        gain=0.2, fractional_threshold=0.05)
    assert isinstance(comp["pixels"].data, torch.Tensor) == on_device
    comp, resid = H(comp["pixels"].data), H(resid["pixels"].data)
    assert comp.shape == resid.shape == (2, 4, 64, 48)
    for chan in range(2):
        for pol in range(4):
            if pol == 2:
                assert not comp[chan, pol].any() and not resid[chan, pol].any()
                continue
            c, r = cleaners.hogbom(dirty[chan, pol], psf[chan, pol], None, 0.2, 0.0, 40, 0.05)
            assert np.array_equal(comp[chan, pol], c) and np.array_equal(resid[chan, pol], r)
            want = cr.hogbom(dirty[chan, pol], psf[chan, pol], None, 0.2, 0.0, 40, 0.05)
            assert np.abs(c - want[0]).max() <= 1e-12 and np.abs(r - want[1]).max() <= 1e-12


def test_deconvolve_cube_default_is_msclean():
    dirty, psf = _cube()
    comp, resid = image.deconvolve_cube(*_cube_images(), niter=10, scales=[0, 3])
    want = cr.msclean(dirty[1, 3], psf[1, 3], None, None, 0.1, 0.0, 10, [0, 3], 0.01)
    assert np.abs(comp["pixels"].data[1, 3] - want[0]).max() <= MSCLEAN_TOL
    assert np.abs(resid["pixels"].data[1, 3] - want[1]).max() <= MSCLEAN_TOL
    assert not comp["pixels"].data[:, 2].any()


@pytest.mark.parametrize("shape,kwargs,rows,cols", [
    ("quarter", {}, slice(17, 48), slice(13, 36)),
    ("no_edge", {"window_edge": 5}, slice(6, 59), slice(6, 43))])
def test_deconvolve_cube_windows(shape, kwargs, rows, cols):
    dirty, psf = _cube()
    comp, resid = image.deconvolve_cube(*_cube_images(), algorithm="hogbom", niter=30, gain=0.2,
                                        window_shape=shape, **kwargs)
    window = np.zeros((64, 48))
    window[rows, cols] = 1.0
    for chan, pol in ((0, 0), (1, 3)):
        want = cr.hogbom(dirty[chan, pol], psf[chan, pol], window, 0.2, 0.0, 30, 0.01)
        assert np.abs(comp["pixels"].data[chan, pol] - want[0]).max() <= 1e-12
        assert np.abs(resid["pixels"].data[chan, pol] - want[1]).max() <= 1e-12
        outside = comp["pixels"].data[chan, pol].copy()
        outside[rows, cols] = 0.0
        assert not outside.any()


def test_deconvolve_cube_honours_psf_support():
    dirty, psf = _cube()
    comp, resid = image.deconvolve_cube(*_cube_images(), algorithm="hogbom", niter=30, gain=0.2,
                                        psf_support=10)
    # the 64 x 48 PSF cut about (nx // 2, ny // 2) as bound_psf_list does
    cut = psf[0, 0][24 - 10:24 + 10, 32 - 10:32 + 10]
    want = cr.hogbom(dirty[0, 0], cut, None, 0.2, 0.0, 30, 0.01)
    full = cr.hogbom(dirty[0, 0], psf[0, 0], None, 0.2, 0.0, 30, 0.01)
    assert np.abs(resid["pixels"].data[0, 0] - want[1]).max() <= 1e-12
    assert np.abs(comp["pixels"].data[0, 0] - want[0]).max() <= 1e-12
    assert np.abs(want[1] - full[1]).max() > 1e-3


def test_sensitivity_reaches_the_cleaner_only_through_deconvolve_list():
    from ska_sdp_func_python_amd.image import deconvolution as dc
    dirty, psf = _cube()
    y, x = np.mgrid[0:64, 0:48]
    sens = np.empty((1, 4, 64, 48))
    sens[:] = 0.3 + 0.7 * np.exp(-((y - 20.0) ** 2 + (x - 30.0) ** 2) / 800.0)
    d1, p1, s1 = _image(np.array(dirty[:1])), _image(np.array(psf[:1])), _image(sens)
    kw = dict(niter=10, scales=[0, 3], gain=0.5)
    plain, _ = image.deconvolve_cube(d1, p1, **kw)
    ignored, _ = image.deconvolve_cube(d1, p1, sensitivity=s1, **kw)
    assert np.array_equal(plain["pixels"].data, ignored["pixels"].data)
    (used,), _ = dc.deconvolve_list([d1], [p1], sensitivity_list=[s1], **kw)
    want = cr.msclean(dirty[0, 0], psf[0, 0], None, sens[0, 0], 0.5, 0.0, 10, [0, 3], 0.01)
    assert np.abs(used["pixels"].data[0, 0] - want[0]).max() <= MSCLEAN_TOL
    assert not np.array_equal(used["pixels"].data[0, 0], plain["pixels"].data[0, 0])


# ---- restore -----------------------------------------------------------------
def _beam(model, sx, sy, theta):
    return image.operations.convert_clean_beam_to_degrees(model, (sx, sy, theta))


def _direct_wrap_convolution(model, sx, sy, theta):
    a = np.cos(theta) ** 2 / (2 * sx**2) + np.sin(theta) ** 2 / (2 * sy**2)
    b = np.sin(2 * theta) / (2 * sx**2) - np.sin(2 * theta) / (2 * sy**2)
    c = np.sin(theta) ** 2 / (2 * sx**2) + np.cos(theta) ** 2 / (2 * sy**2)
    size = int(np.ceil(8 * max(sx, sy)))
    size += 1 - size % 2
    half = size // 2
    ny, nx = model.shape
    out = np.zeros((ny, nx))
    for py, px in zip(*np.nonzero(model)):
        for dy in range(-half, half + 1):
            for dx in range(-half, half + 1):
                out[(py + dy) % ny, (px + dx) % nx] += model[py, px] * np.exp(
                    -(a * dx * dx + b * dx * dy + c * dy * dy))
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
def test_restore_cube_matches_direct_wrap_convolution(on_device):
    model = np.zeros((1, 1, 40, 36))
    model[0, 0, 20, 17], model[0, 0, 8, 30], model[0, 0, 39, 1] = 1.0, -0.6, 0.8  # last one wraps
    resid = np.random.default_rng(3).normal(0, 0.01, model.shape)
    sx, sy, theta = 1.5, 2.5, np.deg2rad(30.0)
    conv = T if on_device else np.array
    mim, rim = _image(conv(model)), _image(conv(resid))
    beam = _beam(mim, sx, sy, theta)
    restored = image.restore_cube(mim, residual=rim, clean_beam=beam)
    assert isinstance(restored["pixels"].data, torch.Tensor) == on_device
    assert restored.attrs["clean_beam"] == beam
    # the beam goes through degrees and back: (bmin, bmaj, bpa) in pixels
    px = image.operations.convert_clean_beam_to_pixels(mim, beam)
    expect = _direct_wrap_convolution(model[0, 0], *px)
    got = H(restored["pixels"].data)[0, 0]
    assert np.abs(got - resid[0, 0] - expect).max() <= 1e-12 * np.abs(expect).max()
    assert expect[0, 1] > 0.3  # the border source wrapped to the first row
    no_resid = image.restore_cube(mim, clean_beam=beam)
    assert np.abs(H(no_resid["pixels"].data)[0, 0] - expect).max() <= 1e-12 * np.abs(expect).max()
    assert np.array_equal(H(mim["pixels"].data), model)  # the model is not touched


@pytest.mark.parametrize("sx,sy,theta_deg", [(1.5, 2.5, 30.0), (2.8, 1.6, -20.0)])
def test_fit_psf_recovers_a_gaussian(sx, sy, theta_deg):
    theta = np.deg2rad(theta_deg)
    y, x = np.mgrid[0:64, 0:64]
    dx, dy = x - 32.0, y - 32.0
    a = np.cos(theta) ** 2 / (2 * sx**2) + np.sin(theta) ** 2 / (2 * sy**2)
    b = np.sin(2 * theta) / (2 * sx**2) - np.sin(2 * theta) / (2 * sy**2)
    c = np.sin(theta) ** 2 / (2 * sx**2) + np.cos(theta) ** 2 / (2 * sy**2)
    psf = _image(T(np.exp(-(a * dx**2 + b * dx * dy + c * dy**2))[None, None]))
    fit = image.fit_psf(psf)
    want = _beam(psf, sx, sy, theta)
    assert fit["bmaj"] == pytest.approx(want["bmaj"], rel=1e-6)
    assert fit["bmin"] == pytest.approx(want["bmin"], rel=1e-6)
    # the position angle of an ellipse is defined modulo 180 degrees
    dpa = (fit["bpa"] - want["bpa"] + 90.0) % 180.0 - 90.0
    assert abs(dpa) <= 1e-6 * 180.0
    restored = image.restore_cube(psf, psf=psf)
    assert restored.attrs["clean_beam"]["bmaj"] == pytest.approx(want["bmaj"], rel=1e-6)


# ---- end to end -----------------------------------------------------------------
def test_invert_then_hogbom_finds_the_sources():
    """invert_ng(dopsf=True) and invert_ng of three point sources feed
    deconvolve_cube: the residual peak falls below 10 % of the dirty peak and
    the three brightest components sit on the source pixels."""
    from ska_sdp_func_python_amd import simulation
    from ska_sdp_func_python_amd.imaging import invert_ng, predict_ng
    vis = simulation.make_visibility("MID", nants=20, ntimes=5, nchan=2, f_lo=1.4e9)
    cell = 0.5 / (2 * simulation.max_uv_lambda(vis))
    model = dm.create_image(128, cell, vis.phasecentre, frequency=1.4e9)
    sources = {(64, 64): 1.0, (40, 90): 0.7, (85, 30): 0.5}
    for (py, px), flux in sources.items():
        model["pixels"].data[0, 0, py, px] = flux
    pv = predict_ng(vis, model)
    dirty, _ = invert_ng(pv, model)
    psf, _ = invert_ng(pv, model, dopsf=True)
    comp, resid = image.deconvolve_cube(dirty, psf, algorithm="hogbom", niter=200, gain=0.1)
    d, c, r = (H(im["pixels"].data)[0, 0] for im in (dirty, comp, resid))
    print("dirty peak", np.abs(d).max(), "residual peak", np.abs(r).max())
    assert np.abs(r).max() < 0.1 * np.abs(d).max()
    brightest = np.argsort(np.abs(c).ravel())[-3:]
    assert {tuple(int(v) for v in np.unravel_index(i, c.shape)) for i in brightest} == set(sources)
