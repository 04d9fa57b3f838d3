"""GPU parity of multi-scale multi-frequency CLEAN (csrc/mfsclean.hip through
image.cleaners.msmfsclean and image.deconvolution) against the reference's
goldens and the numpy restatement (tests/mfsclean_restatement.py).

Tolerances
  numpy input: the set-up is the host's numpy, the minor cycle the same
  arithmetic in the same order, so only fp64 rounding may differ:
  1e-12 * max|dirty| on model and residual, the project's bound for that
  (tests/test_gpu_clean.py); with contraction off in mfsclean.hip the match is
  expected to be exact.
  device input: the only extra difference is the set-up FFT (torch.fft on the
  device instead of numpy.fft).  Measured on the CPU, the restatement run with
  numpy.fft against the same run with torch.fft differs over F1 .. F11 by at
  most 2.5e-14 (F1's model, whose higher moments come through the inverse
  Hessian; residuals 1.3e-15 at most); 10x that is allowed.
  The per-channel lists of mmclean_kernel_list are sum_k w_k * moment[k] with
  w_k = ((nu - nu_ref) / nu_ref)^k, so their tolerance is the moments' times
  sum_k max|w_k|.
"""

import numpy as np
import pytest
import torch

import mfsclean_restatement as mr
from test_mfsclean_cpu import CASES, args_of, channel_images, load_case, restated
from conftest import golden
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd import image
from ska_sdp_func_python_amd.image import cleaners
from ska_sdp_func_python_amd.image import taylor_terms as tt

pytestmark = pytest.mark.gpu
FFT_DIFF = 2.5e-14  # see the module docstring
DEVICE_TOL = 10 * FFT_DIFF


def T(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=float), device="cuda:0")


def H(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def run(c, on_device, **over):
    conv = T if on_device else (lambda a: a)
    c = dict(c, **over)
    out = cleaners.msmfsclean_run(conv(c["dirty"]), conv(c["psf"]), conv(c["window"]), conv(c["sens"]),
                                  c["gain"], c["thresh"], c["niter"], c["scales"], c["fracthresh"],
                                  c["findpeak"])
    assert all(isinstance(a, torch.Tensor) == on_device for a in out[:2])
    return H(out[0]), H(out[1]), out[2]


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", CASES)
def test_msmfsclean_golden(name, on_device):
    c = load_case(name)
    model, res, info = run(c, on_device)
    tol = DEVICE_TOL if on_device else 1e-12 * np.abs(c["dirty"]).max()
    print(name, "model", np.abs(model - c["model"]).max(), "res", np.abs(res - c["residual"]).max(),
          "bit-equal", np.array_equal(model, c["model"]) and np.array_equal(res, c["residual"]), info)
    assert model.shape == res.shape == c["dirty"].shape
    assert np.array_equal(model != 0, c["model"] != 0)
    assert info["niter"] == restated(name)[2]
    assert info["scale_counts"] == restated(name)[3]
    assert info["stop"] == ("threshold" if name == "F10" else "niter")
    assert np.abs(model - c["model"]).max() <= tol
    assert np.abs(res - c["residual"]).max() <= tol
    if name == "F1":
        conv = T if on_device else (lambda a: a)
        plain = cleaners.msmfsclean(conv(c["dirty"]), conv(c["psf"]), None, None, c["gain"],
                                    c["thresh"], c["niter"], c["scales"], c["fracthresh"])
        assert len(plain) == 2 and np.array_equal(H(plain[0]), model) and np.array_equal(H(plain[1]), res)


def test_algorithm1_is_rascil():
    c = load_case("F1")
    a = run(c, False)
    b = run(c, False, findpeak="Algorithm1")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    casa = run(c, False, findpeak="CASA")
    assert not np.array_equal(a[0], casa[0])


def _tie_case():
    """Two equal peaks in different tiles, delta PSF moments."""
    dirty = np.zeros((2, 70, 70))
    dirty[0, 3, 66] = dirty[0, 40, 5] = 1.0
    dirty[1, 3, 66] = dirty[1, 40, 5] = 0.25
    psf = np.zeros((4, 16, 16))
    psf[:, 8, 8] = [1.0, 0.1, 0.05, 0.01]
    return dirty, psf


def test_exact_tie_takes_the_first_index_across_tiles():
    """Model and residual equal the restatement's bit for bit, so the lower
    flat index wins every tie.  After an even number of cycles both peaks have
    had the same share, so niter = 5 is run as well: there the first peak is
    one component ahead."""
    dirty, psf = _tie_case()
    for niter in (6, 5):
        want = mr.msmfsclean(dirty, psf, None, None, 0.5, 0.0, niter, [0], 0.0)
        assert want[0][0, 3, 66] != 0 and want[0][0, 40, 5] != 0
        assert (want[0][0, 3, 66] > want[0][0, 40, 5]) == (niter == 5)
        model, res, info = cleaners.msmfsclean_run(dirty, psf, None, None, 0.5, 0.0, niter, [0], 0.0)
        assert np.array_equal(model, want[0]) and np.array_equal(res, want[1])
        assert info["niter"] == want[2] == niter and info["scale_counts"] == want[3]


def test_exact_tie_across_scales_takes_the_lower_scale():
    """The same pair with scales [0, 0] (two identical scale planes)."""
    dirty, psf = _tie_case()
    for niter in (6, 5):
        want = mr.msmfsclean(dirty, psf, None, None, 0.5, 0.0, niter, [0, 0], 0.0)
        model, res, info = cleaners.msmfsclean_run(dirty, psf, None, None, 0.5, 0.0, niter, [0, 0], 0.0)
        assert np.array_equal(model, want[0]) and np.array_equal(res, want[1])
        assert info["scale_counts"] == want[3] == [niter, 0]


def test_limits_are_rejected():
    from ska_sdp_func_python_amd import kernels
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda:0")
    eye = lambda s, t: np.tile(np.eye(t), (s, 1, 1))
    with pytest.raises(ValueError, match="nmoment must be 1..4"):
        kernels.mfsclean_plane(z(1, 5, 8, 8), z(5, 8, 8), z(1, 1, 9, 4, 4), z(1, 4, 4), eye(1, 5),
                               eye(1, 5), 0.5, 0.0, 1)
    with pytest.raises(ValueError, match="nscales must be 1..16"):
        kernels.mfsclean_plane(z(17, 1, 8, 8), z(1, 8, 8), z(17, 17, 1, 4, 4), z(17, 4, 4), eye(17, 1),
                               eye(17, 1), 0.5, 0.0, 1)
    with pytest.raises(ValueError, match="ssmmpsf must be"):
        kernels.mfsclean_plane(z(1, 2, 8, 8), z(2, 8, 8), z(1, 1, 4, 4, 4), z(1, 4, 4), eye(1, 2),
                               eye(1, 2), 0.5, 0.0, 1)


# ---- mmclean_kernel_list -------------------------------------------------------------
def _cube_image(cube, f0, bw):
    im = dm.create_image(max(cube.shape[2:]), 0.001, dm.SkyCoord(0.2, -0.7), frequency=f0,
                         channel_bandwidth=bw, nchan=cube.shape[0])
    im["pixels"].data = cube
    im.attrs["_polarisation_frame"] = "stokesIQ"
    return im


def _list_tolerance(on_device, dirty, psf, f0, bw, nmoment):
    nchan = dirty.shape[0]
    freq = f0 + bw * np.arange(nchan)
    w = np.abs(freq - freq[nchan // 2]) / freq[nchan // 2]
    weights = sum(w.max() ** k for k in range(nmoment))
    # what the cleaner sees as dirty moment 0: the sum over channels over the PSF moments' peak
    moment_tol = DEVICE_TOL if on_device else 1e-12 * np.abs(dirty.sum(0)).max() / psf.sum(0).max()
    return moment_tol * weights


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("algorithm", ["msmfsclean", "mfsmsclean", "mmclean"])
def test_list_golden(algorithm, on_device):
    inp, out = golden("mfsclean_L1_inputs.npz"), golden("mfsclean_L1.npz")
    f0, bw = float(inp["f0"]), float(inp["bw"])
    conv = T if on_device else np.array
    kwargs = dict(algorithm=algorithm, nmoment=int(out["nmoment"]), niter=int(out["niter"]),
                  gain=float(out["gain"]), fractional_threshold=float(out["fractional_threshold"]),
                  threshold=float(out["threshold"]), scales=[float(s) for s in out["scales"]],
                  window_shape=str(out["window_shape"]))
    tol = _list_tolerance(on_device, inp["dirty"], inp["psf"], f0, bw, kwargs["nmoment"])
    comp_list, resid_list = image.deconvolve_list(channel_images(conv(inp["dirty"]), f0, bw),
                                                  channel_images(conv(inp["psf"]), f0, bw), **kwargs)
    comp_cube, resid_cube = image.deconvolve_cube(_cube_image(conv(inp["dirty"]), f0, bw),
                                                  _cube_image(conv(inp["psf"]), f0, bw), **kwargs)
    assert len(comp_list) == len(resid_list) == 7
    assert isinstance(comp_cube["pixels"].data, torch.Tensor) == on_device
    comp = np.concatenate([H(im["pixels"].data) for im in comp_list])
    resid = np.concatenate([H(im["pixels"].data) for im in resid_list])
    print(algorithm, "comp", np.abs(comp - out["comp"]).max(), "resid",
          np.abs(resid - out["residual"]).max(), "tol", tol)
    assert np.abs(comp - out["comp"]).max() <= tol
    assert np.abs(resid - out["residual"]).max() <= tol
    assert comp[:, 1].any()  # polarisation 1, whose PSF planes are zero, is cleaned with pol 0's
    assert np.array_equal(H(comp_cube["pixels"].data), comp)
    assert np.array_equal(H(resid_cube["pixels"].data), resid)
    assert comp_cube.image_acc.wcs.wcs.ctype[3] == "FREQ"


# ---- end to end --------------------------------------------------------------------------
def test_invert_then_mmclean_finds_the_sources():
    """Five channels of three point sources with spectral indices, predicted
    and inverted per channel, feed deconvolve_cube(algorithm="mmclean"): the
    result matches the restatement run on the same dirty and PSF cubes, and
    the brightest moment-0 components (channel nchan // 2, whose Taylor
    weights are 1, 0) sit on the source pixels."""
    from ska_sdp_func_python_amd import simulation
    from ska_sdp_func_python_amd.imaging import invert_ng, predict_ng
    nchan, f_lo, f_hi = 5, 1.0e9, 1.4e9
    vis = simulation.make_visibility("MID", nants=20, ntimes=5, nchan=nchan, f_lo=f_lo, f_hi=f_hi)
    cell = 0.5 / (2 * simulation.max_uv_lambda(vis))
    bw = (f_hi - f_lo) / (nchan - 1)
    model = dm.create_image(128, cell, vis.phasecentre, frequency=f_lo, channel_bandwidth=bw,
                            nchan=nchan)
    sources = {(64, 64): (1.0, -0.7), (40, 90): (0.7, 0.3), (85, 30): (0.5, -1.2)}
    freq = f_lo + bw * np.arange(nchan)
    for (py, px), (flux, alpha) in sources.items():
        model["pixels"].data[:, 0, py, px] = flux * (freq / freq[nchan // 2]) ** alpha
    pv = predict_ng(vis, model)
    dirty, _ = invert_ng(pv, model)
    psf, _ = invert_ng(pv, model, dopsf=True)
    for im in (dirty, psf):
        im["pixels"].data = T(H(im["pixels"].data))
    comp, resid = image.deconvolve_cube(dirty, psf, algorithm="mmclean", nmoment=2, niter=200)
    assert isinstance(comp["pixels"].data, torch.Tensor)

    d, p = H(dirty["pixels"].data), H(psf["pixels"].data)
    dirty_list, psf_list = channel_images(d, f_lo, bw), channel_images(p, f_lo, bw)
    for host, dev in zip(dirty_list, image.deconvolution._scatter_channels(dirty)):
        assert host.image_acc.wcs.wcs.crval[3] == dev.image_acc.wcs.wcs.crval[3]
    dm_ = tt.calculate_image_list_frequency_moments(dirty_list, nmoment=2)
    pm = tt.calculate_image_list_frequency_moments(psf_list, nmoment=4)["pixels"].data
    peak = pm.max()
    want = mr.msmfsclean(dm_["pixels"].data[:, 0] / peak, pm[:, 0] / peak, None, None, 0.7, 0.0, 200,
                         [0, 3, 10, 30], 0.01)
    print("cycles", want[2], "scale counts", want[3])
    tol = _list_tolerance(True, d, p, f_lo, bw, 2)
    for moments, got in ((want[0], comp), (want[1], resid)):
        dm_["pixels"].data = moments[:, None]
        rebuilt = tt.calculate_image_list_from_frequency_taylor_terms(dirty_list, dm_)
        expect = np.concatenate([im["pixels"].data for im in rebuilt])
        print("difference", np.abs(H(got["pixels"].data) - expect).max(), "tol", tol)
        assert np.abs(H(got["pixels"].data) - expect).max() <= tol
    c0 = H(comp["pixels"].data)[nchan // 2, 0]
    brightest = np.argsort(np.abs(c0).ravel())[-3:]
    assert {tuple(int(v) for v in np.unravel_index(i, c0.shape)) for i in brightest} == set(sources)
