"""Image-plane cleaners on 2-D arrays (reference
src/ska_sdp_func_python/image/cleaners.py): ``hogbom`` (:23-133) and
``msclean`` (:279-470) with the scale-stack helpers (:473-562).

The minor cycles run on the device in ``kernels.clean_plane``
(csrc/clean.hip): the full-image argmax and the shifted PSF subtraction of
every cycle, in fp64 and in the reference's arithmetic order.  numpy input
gives numpy output, device tensors give device tensors.

The msclean set-up (scale stacks, the S + S^2 FFT convolutions, the coupling
matrix, the window stack) is not the hot path: it is numpy on the host for
numpy input -- the reference's own operations, so the minor cycles start from
its bits -- and ``torch.fft`` in fp64 for device input.
"""

import logging

import numpy
import torch

from .. import _device, kernels

__all__ = ["hogbom", "msclean", "hogbom_run", "msclean_run", "create_scalestack",
           "convolve_scalestack", "convolve_convolve_scalestack", "spheroidal_function"]

log = logging.getLogger("func-python-logger")


def _dev64(a):
    return _device.to_dev(a, torch.float64).contiguous()


def hogbom_run(dirty, psf, window, gain, thresh, niter, fracthresh, prefix=""):
    """``hogbom`` that also reports what the minor cycle did: returns
    (comps, residual, {"niter": cycles run, "stop": "niter" | "threshold"})."""
    assert 0.0 < gain < 2.0
    assert niter > 0
    res = _dev64(dirty).clone()[None]
    dpsf = _dev64(psf)
    absolutethresh = max(thresh, fracthresh * float(res.abs().max()))
    pmax = float(dpsf.max())
    numpy.testing.assert_approx_equal(pmax, 1.0, err_msg=f"PSF does not have unit peak {pmax}")
    comps = torch.zeros_like(res[0])
    win = None if window is None else _dev64(window)[None]
    log.info("hogbom %s This minor cycle will stop at %d iterations or peak < %.6f (Jy/beam)",
             prefix, niter, absolutethresh)
    done, stop = kernels.clean_plane("hogbom", res, dpsf[None, None], comps, gain, pmax,
                                     absolutethresh, niter, window=win)
    log.info("hogbom %s End of minor cycle: %d iterations (%s)", prefix, done, stop)
    return (_device.like_input(comps, dirty), _device.like_input(res[0], dirty),
            {"niter": done, "stop": stop})


def hogbom(dirty, psf, window, gain, thresh, niter, fracthresh, prefix=""):
    """Clean the point spread function from a dirty image (Hogbom 1974).

    :param dirty: dirty image [ny, nx]
    :param psf: point spread function (unit peak), any size
    :param window: array multiplying the search values, or None
    :param gain: loop gain
    :param thresh: stop once |residual at the peak| < 0.9 * max(thresh, fracthresh * max|dirty|)
    :param niter: maximum number of components
    :param fracthresh: fractional threshold
    :return: component image, residual image
    """
    return hogbom_run(dirty, psf, window, gain, thresh, niter, fracthresh, prefix)[:2]


def msclean_run(dirty, psf, window, sensitivity, gain, thresh, niter, scales, fracthresh,
                prefix=""):
    """``msclean`` that also reports what the minor cycle did: returns (comps,
    residual, {"niter": cycles, "stop": "niter" | "threshold" | "zero"})."""
    assert 0.0 < gain < 2.0
    assert niter > 0
    assert len(scales) > 0
    on_dev = _device.is_device(dirty)
    if on_dev:
        dirty_, psf_ = _dev64(dirty), _dev64(psf)
        window_ = None if window is None else _dev64(window)
    else:
        dirty_, psf_ = numpy.asarray(dirty, dtype=float), numpy.asarray(psf, dtype=float)
        window_ = None if window is None else numpy.asarray(window, dtype=float)
    pmax = float(psf_.max())
    assert pmax > 0.0
    lpsf = psf_ / pmax
    ldirty = dirty_ / pmax

    ns = len(scales)
    scalestack = create_scalestack([ns, ldirty.shape[0], ldirty.shape[1]], scales, norm=True)
    pscalestack = create_scalestack([ns, lpsf.shape[0], lpsf.shape[1]], scales, norm=True)
    # how far the scale kernels reach from the PSF origin: the component update
    # visits only that part of the patch
    nz = numpy.nonzero(pscalestack.any(axis=0))
    extent = int(max(abs(nz[0] - lpsf.shape[0] // 2).max(), abs(nz[1] - lpsf.shape[1] // 2).max(), 1))
    if on_dev:
        scalestack, pscalestack = _dev64(scalestack), _dev64(pscalestack)
    res_scalestack = convolve_scalestack(scalestack, ldirty)
    psf_scalescalestack = convolve_convolve_scalestack(pscalestack, lpsf)
    coupling = [float(psf_scalescalestack[s, s].max()) for s in range(ns)]
    log.info("msclean %s: Coupling matrix diagonal = %s", prefix, coupling)

    windowstack = None
    if window_ is not None:
        smooth = convolve_scalestack(scalestack, window_)
        windowstack = (smooth > 0.9).to(torch.float64) if on_dev else (smooth > 0.9).astype(float)
        assert float(windowstack.sum()) > 0

    maxabs = float(abs(res_scalestack[0]).max())
    absolutethresh = max(thresh, fracthresh * maxabs)
    log.info("msclean %s: This minor cycle will stop at %d iterations or peak < %.6f (Jy/beam)",
             prefix, niter, absolutethresh)

    res = _dev64(res_scalestack)
    comps = torch.zeros_like(res[0])
    done, stop = kernels.clean_plane(
        "msclean", res, _dev64(psf_scalescalestack), comps, gain, pmax, absolutethresh, niter,
        window=None if windowstack is None else _dev64(windowstack),
        sensitivity=None if sensitivity is None else _dev64(sensitivity),
        coupling_diag=coupling, scale_kernels=_dev64(pscalestack), scale_extent=extent)
    log.info("msclean %s: End of minor cycle: %d iterations (%s)", prefix, done, stop)
    return (_device.like_input(comps, dirty), _device.like_input(pmax * res[0], dirty),
            {"niter": done, "stop": stop})


def msclean(dirty, psf, window, sensitivity, gain, thresh, niter, scales, fracthresh, prefix=""):
    """Multi-scale CLEAN (Cornwell 2008).

    :param dirty: dirty image [ny, nx]
    :param psf: point spread function, any size
    :param window: clean window or None; each scale searches where the window
                   smoothed by that scale exceeds 0.9
    :param sensitivity: inverse noise image or None.  As in the reference the
                   peak of each scale is found on residual * sensitivity^2 and
                   the scales are compared on residual * sensitivity
    :param gain: loop gain
    :param thresh: stop once the peak is below 0.9 * max(thresh, fracthresh *
                   max|dirty smoothed by scale 0|)
    :param niter: maximum number of components
    :param scales: scale sizes in pixels
    :param fracthresh: fractional threshold
    :return: component image, residual image
    """
    return msclean_run(dirty, psf, window, sensitivity, gain, thresh, niter, scales, fracthresh,
                       prefix)[:2]


# Schwab (1984, Indirect Imaging) rational approximation of the prolate
# spheroidal wave function, m = 6, alpha = 1, on [0, 0.75) and [0.75, 1].
_PSWF_P = ((8.203343e-2, -3.644705e-1, 6.278660e-1, -5.335581e-1, 2.312756e-1),
           (4.028559e-3, -3.697768e-2, 1.021332e-1, -1.201436e-1, 6.412774e-2))
_PSWF_Q = ((1.0000000, 8.212018e-1, 2.078043e-1), (1.0000000, 9.599102e-1, 2.918724e-1))


def spheroidal_function(vnu):
    """Prolate spheroidal wave function at ``vnu`` in [0, 1] (0 outside)."""
    if 0.0 <= vnu < 0.75:
        part, nuend = 0, 0.75
    elif 0.75 <= vnu <= 1.0:
        part, nuend = 1, 1.0
    else:
        return 0.0
    delnusq = vnu**2 - nuend**2
    top, bot = _PSWF_P[part][0], _PSWF_Q[part][0]
    for k in range(1, 5):
        top += _PSWF_P[part][k] * delnusq**k
    for k in range(1, 3):
        bot += _PSWF_Q[part][k] * delnusq**k
    return max(top / bot, 0.0) if bot != 0.0 else 0.0


def create_scalestack(scaleshape, scales, norm=True):
    """Cube [len(scales), n0, n1] of the scale kernels (host numpy): a tapered
    paraboloid of the given width in pixels, a delta for scale 0, each centred
    at pixel ceil(n / 2) -- not the PSF's n // 2, which differs for odd n."""
    assert scaleshape[0] == len(scales)
    basis = numpy.zeros(scaleshape)
    cen0 = int(numpy.ceil(float(scaleshape[1]) / 2.0))
    cen1 = int(numpy.ceil(float(scaleshape[2]) / 2.0))
    for iscale, scale in enumerate(scales):
        if scale > 0.0:
            half = int(numpy.ceil(scale / 2.0))
            rscale2 = 1.0 / (float(scale) / 2.0) ** 2
            for i1 in range(cen1 - half - 1, cen1 + half + 1):
                for i0 in range(cen0 - half - 1, cen0 + half + 1):
                    f0, f1 = float(i0 - cen0), float(i1 - cen1)
                    r = numpy.sqrt(rscale2 * (f0 * f0 + f1 * f1))
                    basis[iscale, i0, i1] = spheroidal_function(r) * (1.0 - r**2)
            basis[basis < 0.0] = 0.0
            if norm:
                basis[iscale] /= numpy.sum(basis[iscale])
        else:
            basis[iscale, cen0, cen1] = 1.0
    return basis


def _fft_ops(a):
    if isinstance(a, torch.Tensor):
        f = torch.fft
        return f.fft2, f.ifft2, f.fftshift, f.ifftshift, torch.conj, lambda z: z.real
    f = numpy.fft
    return f.fft2, f.ifft2, f.fftshift, f.ifftshift, numpy.conjugate, numpy.real


def convolve_scalestack(scalestack, img):
    """``img`` correlated with every plane of ``scalestack`` by FFT; numpy in,
    numpy out, device tensors in, device tensor out (torch.fft, fp64)."""
    fft2, ifft2, shift, ishift, conj, real = _fft_ops(img)
    ximg = shift(fft2(shift(img)))
    planes = []
    for iscale in range(scalestack.shape[0]):
        xscale = shift(fft2(shift(scalestack[iscale])))
        planes.append(real(ishift(ifft2(ishift(ximg * conj(xscale))))))
    return torch.stack(planes) if isinstance(img, torch.Tensor) else numpy.array(planes)


def convolve_convolve_scalestack(scalestack, img):
    """``img`` smoothed by every pair of scales: [nscales, nscales, n0, n1]."""
    fft2, ifft2, shift, ishift, conj, real = _fft_ops(img)
    ns = scalestack.shape[0]
    ximg = shift(fft2(shift(img)))
    xscale = [shift(fft2(shift(scalestack[s]))) for s in range(ns)]
    rows = []
    for s in range(ns):
        row = [real(ishift(ifft2(ishift(ximg * xscale[p] * conj(xscale[s]))))) for p in range(ns)]
        rows.append(torch.stack(row) if isinstance(img, torch.Tensor) else numpy.array(row))
    return torch.stack(rows) if isinstance(img, torch.Tensor) else numpy.array(rows)
