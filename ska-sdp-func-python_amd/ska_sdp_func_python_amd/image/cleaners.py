"""Image-plane cleaners on 2-D arrays and moment stacks (reference
src/ska_sdp_func_python/image/cleaners.py): ``hogbom`` (:23-133),
``hogbom_complex`` (:136-232, Q + iU cleaned as one complex image), ``msclean``
(:279-470) with the scale-stack helpers (:473-562), and ``msmfsclean``
(:686-898) with its set-up helpers (:1034-1104).

The minor cycles run on the device in ``kernels.clean_plane`` and
``kernels.clean_plane_complex`` (csrc/clean.hip) and
``kernels.mfsclean_plane`` (csrc/mfsclean.hip): the
full-image search and the shifted PSF subtraction of every cycle, in fp64 and
in the reference's arithmetic order.  numpy input gives numpy output, device
tensors give device tensors.

The set-up (scale stacks, the FFT convolutions -- S + S^2 for msclean,
S T + S^2 (2T - 1) for msmfsclean --, the coupling matrix or Hessians, the
window stack) is not the hot path: it is numpy on the host for numpy input --
the reference's own operations, so the minor cycles start from its bits --
and ``torch.fft`` in fp64 for device input.
"""

import logging

import numpy
import torch

from .. import _device, kernels

__all__ = ["hogbom", "hogbom_complex", "msclean", "msmfsclean", "hogbom_run", "hogbom_complex_run",
           "msclean_run", "msmfsclean_run",
           "create_scalestack", "convolve_scalestack", "convolve_convolve_scalestack",
           "calculate_scale_moment_residual", "calculate_scale_scale_moment_moment_psf",
           "calculate_scale_inverse_moment_moment_hessian", "spheroidal_function"]

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


def hogbom_complex_run(dirty_q, dirty_u, psf_q, psf_u, window, gain, thresh, niter, fracthresh):
    """``hogbom_complex`` that also reports what the minor cycle did: returns
    (comps_q, comps_u, res_q, res_u, {"niter": cycles run, "stop": "niter" | "threshold"})."""
    assert 0.0 < gain < 2.0
    assert niter > 0
    dpsf, dpsf_u = _dev64(psf_q), _dev64(psf_u)
    assert dpsf.shape == dpsf_u.shape and bool((dpsf == dpsf_u).all())
    pmax = float(dpsf.max())
    assert pmax > 0.0
    res = torch.stack([_dev64(dirty_q), _dev64(dirty_u)])
    absolutethresh = max(thresh, fracthresh * float(torch.hypot(res[0], res[1]).max()))
    comps = torch.zeros_like(res)
    win = None if window is None else _dev64(window)
    log.info("hogbom_complex: This minor cycle will stop at %d iterations or peak < %s", niter,
             absolutethresh)
    done, stop = kernels.clean_plane_complex(res, dpsf, comps, gain, pmax, absolutethresh, niter,
                                             window=win)
    log.info("hogbom_complex: End of minor cycle: %d iterations (%s)", done, stop)
    return (_device.like_input(comps[0], dirty_q), _device.like_input(comps[1], dirty_q),
            _device.like_input(res[0], dirty_q), _device.like_input(res[1], dirty_q),
            {"niter": done, "stop": stop})


def hogbom_complex(dirty_q, dirty_u, psf_q, psf_u, window, gain, thresh, niter, fracthresh):
    """Complex Hogbom CLEAN of polarised data (Pratley & Johnston-Hollitt
    2016): Stokes Q and U are cleaned together as P = Q + iU, the peak is
    searched on |P|, so that the result does not depend on the polarisation
    angle.

    :param dirty_q: dirty Q image [ny, nx]
    :param dirty_u: dirty U image [ny, nx]
    :param psf_q: point spread function of Q, any size; its maximum must be
                  positive but need not be 1 (the components are divided by it)
    :param psf_u: point spread function of U, which must equal ``psf_q``
    :param window: array multiplying Q and U in the search, or None
    :param gain: loop gain
    :param thresh: stop once |P| at the peak, after the subtraction, is below
                   max(thresh, fracthresh * max|P|) -- without the factor 0.9
                   of ``hogbom``
    :param niter: maximum number of components
    :param fracthresh: fractional threshold
    :return: Q components, U components, Q residual, U residual

    Arithmetic (csrc/clean.hip, ``kernels.clean_plane_complex``): the search
    key is hypot(q * w, u * w), the first maximum in row-major order wins, and
    the component is (P[peak] * gain) * (1 / pmax) -- numpy's division of a
    complex scalar by a real one.
    """
    return hogbom_complex_run(dirty_q, dirty_u, psf_q, psf_u, window, gain, thresh, niter,
                              fracthresh)[:4]


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


def msmfsclean_run(dirty, psf, window, sensitivity, gain, thresh, niter, scales, fracthresh,
                   findpeak="RASCIL", prefix=""):
    """``msmfsclean`` that also reports what the minor cycle did: returns
    (m_model, residual, {"niter": cycles, "stop": "niter" | "threshold",
    "scale_counts": cycles that chose each scale})."""
    assert 0.0 < gain < 2.0
    assert niter > 0
    assert len(scales) > 0
    on_dev = _device.is_device(dirty)
    if on_dev:
        conv = _dev64
    else:
        conv = lambda a: numpy.asarray(a, dtype=float)
    dirty_, psf_ = conv(dirty), conv(psf)
    window_ = None if window is None else conv(window)
    pmax = float(psf_.max())
    assert pmax > 0.0
    lpsf = psf_ / pmax
    ldirty = dirty_ / pmax
    nmoment = ldirty.shape[0]
    if nmoment > 1:
        assert psf_.shape[0] == 2 * nmoment

    ns = len(scales)
    scalestack = create_scalestack([ns, ldirty.shape[1], ldirty.shape[2]], scales, norm=True)
    pscalestack = create_scalestack([ns, lpsf.shape[1], lpsf.shape[2]], scales, norm=True)
    # how far the scale kernels reach from the PSF origin: the model update
    # visits only that part of the patch
    nz = numpy.nonzero(pscalestack.any(axis=0))
    extent = int(max(abs(nz[0] - lpsf.shape[1] // 2).max(), abs(nz[1] - lpsf.shape[2] // 2).max(), 1))
    if on_dev:
        scalestack, pscalestack = _dev64(scalestack), _dev64(pscalestack)
    smresidual = calculate_scale_moment_residual(ldirty, scalestack)
    ssmmpsf = calculate_scale_scale_moment_moment_psf(lpsf, pscalestack)
    hsmmpsf, ihsmmpsf = calculate_scale_inverse_moment_moment_hessian(ssmmpsf)
    for s in range(ns):
        log.debug("mmclean %s: Moment-moment coupling matrix[scale %d] =\n %s", prefix, s, hsmmpsf[s])

    windowstack = None
    if window_ is not None:
        smooth = convolve_scalestack(scalestack, window_)
        windowstack = (smooth > 0.9).to(torch.float64) if on_dev else (smooth > 0.9).astype(float)

    if sensitivity is not None:
        sensitivity = conv(sensitivity)
        if sensitivity.ndim == 3:
            # the reference broadcasts [nmoment, ny, nx] against the 2-D search
            # field and takes the maximum over the moments too; rounding is
            # monotone, so max_m |s_m * f| = |max_m |s_m| * f| exactly
            sensitivity = abs(sensitivity).amax(0) if on_dev else abs(sensitivity).max(0)

    maxabs = float(abs(smresidual[0, 0]).max())
    absolutethresh = max(thresh, fracthresh * maxabs)
    log.info("mmclean %s: This minor cycle will stop at %d iterations or peak < %.6f (Jy/beam)",
             prefix, niter, absolutethresh)

    res = _dev64(smresidual)
    m_model = torch.zeros_like(res[0])
    done, stop, counts = kernels.mfsclean_plane(
        res, m_model, _dev64(ssmmpsf), _dev64(pscalestack), hsmmpsf, ihsmmpsf, gain, absolutethresh,
        niter, findpeak=findpeak,
        windowstack=None if windowstack is None else _dev64(windowstack),
        sensitivity=None if sensitivity is None else _dev64(sensitivity), scale_extent=extent)
    log.info("mmclean %s: End of minor cycles: %d iterations (%s), scale counts %s", prefix, done,
             stop, counts)
    return (_device.like_input(m_model, dirty), _device.like_input(pmax * res[0], dirty),
            {"niter": done, "stop": stop, "scale_counts": counts})


def msmfsclean(dirty, psf, window, sensitivity, gain, thresh, niter, scales, fracthresh,
               findpeak="RASCIL", prefix=""):
    """Multi-scale multi-frequency CLEAN (Rau & Cornwell 2011, Algorithm 1;
    the image-plane part) on frequency moments.

    :param dirty: dirty moment images [nmoment, ny, nx], nmoment <= 4
    :param psf: PSF moment images [2 * nmoment, py, px] ([1 or more, py, px]
                for nmoment 1, of which moment 0 is used), any size
    :param window: clean window [ny, nx] or None.  Each scale's window is the
                window smoothed by that scale, where it exceeds 0.9.  As in
                the reference it (and the sensitivity) only weigh the choice
                between scales: the pixel of each scale is the peak of the
                unweighted search image
    :param sensitivity: inverse noise image [ny, nx] or [nmoment, ny, nx], or None
    :param gain: loop gain
    :param thresh: stop once |moment 0 of the peak's principal solution| <
                max(thresh, fracthresh * max|dirty moment 0 smoothed by scale 0|)
    :param niter: maximum number of components
    :param scales: scale sizes in pixels (at most 16)
    :param fracthresh: fractional threshold
    :param findpeak: "CASA" searches the chi-squared decrease, "RASCIL",
                "Algorithm1" and anything else moment 0 of the principal solution
    :return: model moment images, residual moment images
    """
    return msmfsclean_run(dirty, psf, window, sensitivity, gain, thresh, niter, scales, fracthresh,
                          findpeak, prefix)[:2]


def _stack(planes, axis=0):
    if isinstance(planes[0], torch.Tensor):
        return torch.stack(planes, dim=axis)
    return numpy.stack(planes, axis=axis)


def calculate_scale_moment_residual(residual, scalestack):
    """Every moment of ``residual`` [nmoment, ny, nx] smoothed by every scale:
    [nscales, nmoment, ny, nx] (Algorithm 1, lines 12 - 17)."""
    return _stack([convolve_scalestack(scalestack, residual[t]) for t in range(residual.shape[0])],
                  axis=1)


def calculate_scale_scale_moment_moment_psf(psf, scalestack):
    """The PSF moments smoothed by every pair of scales (Algorithm 1, lines 3 - 5),
    in compact form: [nscales, nscales, 2 * nmoment - 1, py, px] with nmoment =
    max(psf.shape[0] // 2, 1).  Plane k is the reference's
    ``ssmmpsf[s, p, t, q]`` for every t + q = k; the reference stores those
    nmoment^2 copies of the 2 * nmoment - 1 distinct arrays."""
    nmoment = max(psf.shape[0] // 2, 1)
    return _stack([convolve_convolve_scalestack(scalestack, psf[k]) for k in range(2 * nmoment - 1)],
                  axis=2)


def calculate_scale_inverse_moment_moment_hessian(scale_scale_moment_moment_psf):
    """Hessian [nscales, nmoment, nmoment] of every scale, read at the PSF
    origin (py // 2, px // 2) of ``ssmmpsf[s, s]``, and its inverse
    (Algorithm 1, lines 7 - 9); host numpy, ``numpy.linalg.inv``.  Takes the
    compact form of ``calculate_scale_scale_moment_moment_psf`` or the
    reference's [nscales, nscales, nmoment, nmoment, py, px]."""
    ssmm = scale_scale_moment_moment_psf
    ns = ssmm.shape[0]
    cy, cx = ssmm.shape[-2] // 2, ssmm.shape[-1] // 2
    centre = ssmm[..., cy, cx]
    centre = centre.cpu().numpy() if isinstance(centre, torch.Tensor) else numpy.asarray(centre)
    nmoment = centre.shape[2] if centre.ndim == 4 else (centre.shape[2] + 1) // 2
    hessian = numpy.zeros([ns, nmoment, nmoment])
    inverse = numpy.zeros([ns, nmoment, nmoment])
    for s in range(ns):
        for t in range(nmoment):
            for q in range(nmoment):
                hessian[s, t, q] = centre[s, s, t, q] if centre.ndim == 4 else centre[s, s, t + q]
        inverse[s] = numpy.linalg.inv(hessian[s])
    return hessian, inverse


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
