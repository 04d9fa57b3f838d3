"""Deconvolution and restore of image cubes (reference
src/ska_sdp_func_python/image/deconvolution.py): ``deconvolve_cube`` /
``deconvolve_list`` (:50-160, :1047-1116) over the Hogbom, multi-scale and
multi-scale multi-frequency cleaners (``mmclean_kernel_list``, :645-824), and
``restore_cube`` / ``restore_list`` / ``fit_psf`` (:949-1189).

Hogbom and msclean clean one channel and polarisation at a time; the
``msmfsclean`` family ("msmfsclean", "mfsmsclean", "mmclean") cleans the
frequency moments of all channels of a polarisation together
(``image.taylor_terms``).  The minor cycles are HIP (``image.cleaners``,
csrc/clean.hip and csrc/mfsclean.hip); the restore is a circular convolution
with ``torch.fft`` on the device.  Pixels may be numpy arrays or device
tensors; outputs follow the dirty (model) image.

The complex Hogbom clean of Q + iU (``cleaners.hogbom_complex``) and its list
driver ``complex_hogbom_kernel_list`` (:394-511) are provided and are called
directly.  The string dispatch ``algorithm="hogbom-complex"`` of
``deconvolve_list`` / ``deconvolve_cube`` is still refused with ``ValueError``
(tests/test_clean_cpu.py pins that): a caller who wants ``psf_support`` or a
window applies ``bound_psf_list`` / ``find_window_list`` first, as
``deconvolve_list`` does for the other cleaners.
"""

import logging
import math

import numpy
import torch

from .. import _device
from ..datamodels import Image, PolarisationFrame
from .cleaners import hogbom, hogbom_complex, msclean, msmfsclean
from .gather_scatter import image_gather_channels, image_scatter_channels
from .operations import convert_clean_beam_to_degrees, convert_clean_beam_to_pixels
from .taylor_terms import (calculate_image_list_frequency_moments,
                           calculate_image_list_from_frequency_taylor_terms)

__all__ = ["deconvolve_cube", "deconvolve_list", "hogbom_kernel_list", "msclean_kernel_list",
           "mmclean_kernel_list", "complex_hogbom_kernel_list", "find_window_list", "bound_psf_list", "check_psf_peak", "common_arguments",
           "restore_cube", "restore_list", "fit_psf"]

log = logging.getLogger("func-python-logger")

_MMCLEAN = ("msmfsclean", "mfsmsclean", "mmclean")
_UNSUPPORTED = ("hogbom-complex",)


def _pixels(im):
    return im["pixels"].data


def _zeros_like(a):
    if isinstance(a, torch.Tensor):
        return torch.zeros(a.shape, dtype=torch.float64, device=a.device)
    return numpy.zeros(a.shape)


def _image_like(data, im):
    return Image.constructor(data=data, polarisation_frame=im.image_acc.polarisation_frame,
                             wcs=im.image_acc.wcs)


def _scatter_channels(im):
    """One single-channel Image per channel (None stays None)."""
    return image_scatter_channels(im)


def _gather_channels(image_list):
    """Concatenate single-channel Images along frequency."""
    return image_gather_channels(image_list)


def deconvolve_list(dirty_list, psf_list, sensitivity_list=None, prefix="", **kwargs):
    """Clean a list of single-channel images.

    :param dirty_list: list of dirty Images [1, npol, ny, nx]
    :param psf_list: list of PSF Images (unit peak)
    :param sensitivity_list: list of sensitivity Images (msclean only), or None
    :param window_shape: "quarter", "no_edge" or None
    :param window_edge: edge width of "no_edge" (16)
    :param mask: window Image, overrides ``window_shape``
    :param psf_support: half width of the PSF box used for the subtraction
    :param algorithm: "msclean" (default), "hogbom", or "msmfsclean" /
        "mfsmsclean" / "mmclean" (see ``mmclean_kernel_list`` for ``nmoment``
        and ``findpeak``)
    :param gain: loop gain (0.1; 0.7 for the msmfsclean family)
    :param niter: minor cycles (100)
    :param threshold: clean threshold (0.0)
    :param fractional_threshold: fractional threshold (0.01)
    :param scales: msclean scales in pixels ([0, 3, 10, 30])
    :return: component image list, residual image list

    A polarisation whose PSF plane has maximum 0 is skipped: its component and
    residual planes are zeros, as in the reference.
    """
    algorithm = kwargs.get("algorithm", "msclean")
    if algorithm in _UNSUPPORTED:
        raise ValueError(f"deconvolve_cube {prefix}: algorithm {algorithm} is not provided")
    if algorithm not in ("msclean", "hogbom") + _MMCLEAN:
        raise ValueError(f"deconvolve_cube {prefix}: Unknown algorithm {algorithm}")

    # window_edge and mask are handed on to find_window_list, which documents
    # them (the reference drops both on this path, so that its "no_edge" always
    # uses the default edge)
    window_list = find_window_list(dirty_list, prefix, window_shape=kwargs.get("window_shape", None),
                                   **{k: kwargs[k] for k in ("window_edge", "mask") if k in kwargs})
    check_psf_peak(psf_list)
    psf_list = bound_psf_list(dirty_list, prefix, psf_list, psf_support=kwargs.get("psf_support", None))
    check_psf_peak(psf_list)

    if algorithm == "msclean":
        return msclean_kernel_list(dirty_list, prefix, psf_list, window_list, sensitivity_list,
                                   **kwargs)
    if algorithm in _MMCLEAN:
        return mmclean_kernel_list(dirty_list, prefix, psf_list, window_list, sensitivity_list,
                                   **kwargs)
    return hogbom_kernel_list(dirty_list, prefix, psf_list, window_list, **kwargs)


def check_psf_peak(psf_list):
    """Assert that every PSF of the list has unit peak (to 6 significant digits)."""
    for ipsf, psf in enumerate(psf_list):
        pmax = float(_pixels(psf).max())
        numpy.testing.assert_approx_equal(
            pmax, 1.0, err_msg=f"check_psf_peak: PSF {ipsf} does not have unit peak {pmax}",
            significant=6)


def find_window_list(dirty_list, prefix, window_shape=None, **kwargs):
    """Clean windows of a list of dirty images.

    :param window_shape: "quarter" (rows qy+1 .. 3qy-1 and columns qx+1 ..
        3qx-1, q = n // 4), "no_edge" (all but ``window_edge`` + 1 leading and
        ``window_edge`` trailing pixels, default 16) or None (no window: returns None)
    :param mask: an Image that replaces the window
    :return: list of window Images, or None
    """
    if window_shape is None:
        return None
    windows = []
    for dirty in dirty_list:
        ny, nx = _pixels(dirty).shape[2:]
        window_array = _zeros_like(_pixels(dirty))
        if window_shape == "quarter":
            qx, qy = nx // 4, ny // 4
            window_array[..., (qy + 1):3 * qy, (qx + 1):3 * qx] = 1.0
        elif window_shape == "no_edge":
            edge = kwargs.get("window_edge", 16)
            window_array[..., (edge + 1):(ny - edge), (edge + 1):(nx - edge)] = 1.0
        else:
            raise ValueError(f"Window shape {window_shape} is not recognized")
        mask = kwargs.get("mask", None)
        if isinstance(mask, Image):
            log.warning("deconvolve_cube %s: Overriding window_shape with mask image", prefix)
            window_array = _pixels(mask)
        windows.append(_image_like(window_array, dirty))
    return windows


def bound_psf_list(dirty_list, prefix, psf_list, psf_support=None):
    """PSFs cut to a box of half width ``psf_support`` about their centre
    (default: half the larger image side); a PSF smaller than that is kept whole.

    As in the reference the x slice is taken about ny // 2 and the y slice
    about nx // 2, which only matters for a non-square PSF.
    """
    psfs = []
    for channel, dirty in enumerate(dirty_list):
        psf = psf_list[channel]
        if psf_support is None:
            psf_support = max(_pixels(dirty).shape[2] // 2, _pixels(dirty).shape[3] // 2)
        pny, pnx = _pixels(psf).shape[2:]
        if psf_support <= pny // 2 and psf_support <= pnx // 2:
            centre = [pny // 2, pnx // 2]
            data = _pixels(psf)[..., (centre[1] - psf_support):(centre[1] + psf_support),
                                (centre[0] - psf_support):(centre[0] + psf_support)]
            psf = _image_like(data, psf)
            log.debug("deconvolve_cube %s: PSF support = +/- %d pixels", prefix, psf_support)
        else:
            log.info("Using entire psf for deconvolution")
        psfs.append(psf)
    return psfs


def common_arguments(**kwargs):
    """fracthresh, gain, niter, thresh, scales from kwargs, with the defaults
    gain 0.1, niter 100, threshold 0.0, fractional_threshold 0.01 and scales
    [0, 3, 10, 30]; ``ValueError`` on values out of range."""
    gain = kwargs.get("gain", 0.1)
    if gain <= 0.0 or gain >= 2.0:
        raise ValueError("Loop gain must be between 0 and 2")
    thresh = kwargs.get("threshold", 0.0)
    if thresh < 0.0:
        raise ValueError("Threshold must be positive or zero")
    niter = kwargs.get("niter", 100)
    if niter < 0:
        raise ValueError("niter must be greater than zero")
    fracthresh = kwargs.get("fractional_threshold", 0.01)
    if fracthresh < 0.0 or fracthresh > 1.0:
        raise ValueError("Fractional threshold should be in range 0.0, 1.0")
    scales = kwargs.get("scales", [0, 3, 10, 30])
    return fracthresh, gain, niter, thresh, scales


def _plane(image_list, channel, pol):
    if image_list is None or image_list[channel] is None:
        return None
    return _pixels(image_list[channel])[0, pol]


def _clean_planes(dirty_list, psf_list, prefix, name, clean_one):
    comp_images, residual_images = [], []
    for channel, dirty in enumerate(dirty_list):
        psf = psf_list[channel]
        comp_array = _zeros_like(_pixels(dirty))
        residual_array = _zeros_like(_pixels(dirty))
        for pol in range(_pixels(dirty).shape[1]):
            if float(_pixels(psf)[0, pol].max()):
                log.info("%s %s: Processing pol %d, channel %d", name, prefix, pol, channel)
                comp_array[0, pol], residual_array[0, pol] = clean_one(
                    _pixels(dirty)[0, pol], _pixels(psf)[0, pol], channel, pol)
            else:
                log.info("%s %s: Skipping pol %d, channel %d", name, prefix, pol, channel)
        comp_images.append(_image_like(comp_array, dirty))
        residual_images.append(_image_like(residual_array, dirty))
    return comp_images, residual_images


def hogbom_kernel_list(dirty_list, prefix, psf_list, window_list, **kwargs):
    """Hogbom clean of every channel and polarisation separately.

    :return: component image list, residual image list
    """
    fracthresh, gain, niter, thresh, _ = common_arguments(**kwargs)
    return _clean_planes(
        dirty_list, psf_list, prefix, "hogbom_kernel_list",
        lambda d, p, channel, pol: hogbom(d, p, _plane(window_list, channel, pol), gain, thresh,
                                          niter, fracthresh, prefix))


def msclean_kernel_list(dirty_list, prefix, psf_list, window_list, sensitivity_list=None, **kwargs):
    """Multi-scale clean of every channel and polarisation separately; the
    search is biased by the sensitivity image where one is given.

    :return: component image list, residual image list
    """
    fracthresh, gain, niter, thresh, scales = common_arguments(**kwargs)
    return _clean_planes(
        dirty_list, psf_list, prefix, "msclean_kernel_list",
        lambda d, p, channel, pol: msclean(d, p, _plane(window_list, channel, pol),
                                           _plane(sensitivity_list, channel, pol), gain, thresh,
                                           niter, scales, fracthresh, prefix))


def complex_hogbom_kernel_list(dirty_list, psf_list, window_list, **kwargs):
    """Complex Hogbom clean of single-channel stokesIQUV images: I and V
    (polarisations 0 and 3) go through ``cleaners.hogbom`` one at a time, Q and
    U (1 and 2) together through ``cleaners.hogbom_complex`` as Q + iU.

    :param dirty_list: list of dirty Images [1, 4, ny, nx]
    :param psf_list: list of PSF Images; Q and U must share one PSF
    :param window_list: list of window Images, or None
    :param gain, niter, threshold, fractional_threshold: see ``deconvolve_list``
    :return: component image list, residual image list (``stokesIQUV``, the
        dirty image's WCS)

    I or V is skipped when its PSF plane has maximum 0, Q and U when the Q PSF
    plane has; Q and U are searched under the window of Q, as in the reference.
    This is called directly: ``deconvolve_list`` does not dispatch to it and
    applies neither ``psf_support`` nor ``window_shape`` for it, so a caller
    who wants them runs ``bound_psf_list`` / ``find_window_list`` first.

    Two deviations from the reference: the output planes are written at
    channel index 0 of every entry (the reference indexes them with the
    position in the list and raises ``IndexError`` from the second entry on),
    and an entry whose polarisation axis is not 4 raises ``ValueError`` before
    any device work.
    """
    fracthresh, gain, niter, thresh, _ = common_arguments(**kwargs)
    for channel, dirty in enumerate(dirty_list):
        if _pixels(dirty).shape[1] != 4:
            raise ValueError(f"complex_hogbom_kernel_list: image {channel} has "
                             f"{_pixels(dirty).shape[1]} polarisations, stokesIQUV needs 4")

    comp_images, residual_images = [], []
    for channel, dirty in enumerate(dirty_list):
        pix, psf = _pixels(dirty)[0], _pixels(psf_list[channel])[0]
        comp_array = _zeros_like(_pixels(dirty))
        residual_array = _zeros_like(_pixels(dirty))
        for pol in (0, 3):
            if float(psf[pol].max()):
                log.info("complex_hogbom_kernel_list: Processing pol %d, channel %d", pol, channel)
                comp_array[0, pol], residual_array[0, pol] = hogbom(
                    pix[pol], psf[pol], _plane(window_list, channel, pol), gain, thresh, niter,
                    fracthresh)
            else:
                log.info("complex_hogbom_kernel_list: Skipping pol %d, channel %d", pol, channel)
        if float(psf[1].max()):
            log.info("complex_hogbom_kernel_list: Processing pol 1 and 2, channel %d", channel)
            (comp_array[0, 1], comp_array[0, 2], residual_array[0, 1],
             residual_array[0, 2]) = hogbom_complex(
                pix[1], pix[2], psf[1], psf[2], _plane(window_list, channel, 1), gain, thresh,
                niter, fracthresh)
        else:
            log.info("complex_hogbom_kernel_list: Skipping pol 1 and 2, channel %d", channel)
        frame, wcs = PolarisationFrame("stokesIQUV"), dirty.image_acc.wcs
        comp_images.append(Image.constructor(data=comp_array, polarisation_frame=frame, wcs=wcs))
        residual_images.append(Image.constructor(data=residual_array, polarisation_frame=frame,
                                                 wcs=wcs))
    return comp_images, residual_images


def mmclean_kernel_list(dirty_list, prefix, psf_list, window_list=None, sensitivity_list=None,
                        **kwargs):
    """Multi-scale multi-frequency clean ("msmfsclean", "mfsmsclean",
    "mmclean"; Rau & Cornwell 2011) of every polarisation: the channels are
    turned into ``nmoment`` frequency moments (Taylor terms), the moments are
    cleaned together by ``cleaners.msmfsclean`` and the cleaned moments are
    turned back into channel images.

    :param nmoment: number of frequency moments (3); ``nchan > 2 * (nmoment - 1)``
        is required, since the PSF needs 2 * nmoment moments (1 for nmoment 1)
    :param gain: loop gain (0.7, unlike the other cleaners)
    :param findpeak: "RASCIL" (default), "Algorithm1" or "CASA"
    :param niter, threshold, fractional_threshold, scales: see ``deconvolve_list``
    :return: component image list, residual image list

    As in the reference, every polarisation is cleaned with the PSF moments of
    polarisation 0 and with the window of channel moment 0; the window moment
    and the sensitivity moments are divided by nchan, the dirty and PSF
    moments by the peak of the PSF moments; all polarisations are skipped only
    if PSF moment 0 of polarisation 0 has maximum 0.
    """
    findpeak = kwargs.get("findpeak", "RASCIL")
    nmoment = kwargs.get("nmoment", 3)
    if not nmoment >= 1:
        raise ValueError("Number of frequency moments must be greater than or equal to one")
    fracthresh, gain, niter, thresh, scales = common_arguments(**kwargs)
    gain = kwargs.get("gain", 0.7)
    if not 0.0 < gain < 2.0:
        raise ValueError("Loop gain must be between 0 and 2")
    nchan = len(dirty_list)
    if not nchan > 2 * (nmoment - 1):
        raise ValueError(f"deconvolve_cube {prefix}: algorithm {kwargs.get('algorithm', 'mmclean')} "
                         f"requires nchan > 2 * (nmoment - 1) ({nchan} > {2 * (nmoment - 1)})")

    moment_image = calculate_image_list_frequency_moments(dirty_list, nmoment=nmoment)
    dirty_taylor = _pixels(moment_image)
    sensitivity_taylor = window_taylor = None
    if sensitivity_list is not None:
        sensitivity_taylor = _pixels(calculate_image_list_frequency_moments(
            sensitivity_list, nmoment=nmoment)) / nchan
    if window_list is not None:
        window_taylor = _pixels(calculate_image_list_frequency_moments(
            window_list, nmoment=nmoment)) / nchan
    psf_taylor = _pixels(calculate_image_list_frequency_moments(
        psf_list, nmoment=2 * nmoment if nmoment > 1 else 1))
    psf_peak = float(psf_taylor.max())
    dirty_taylor = dirty_taylor / psf_peak
    psf_taylor = psf_taylor / psf_peak
    log.info("mmclean_kernel_list %s: Shape of Dirty moments image %s, of PSF moments image %s",
             prefix, tuple(dirty_taylor.shape), tuple(psf_taylor.shape))

    comp_array = _zeros_like(dirty_taylor)
    residual_array = _zeros_like(dirty_taylor)
    for pol in range(dirty_taylor.shape[1]):
        # always the moment 0, polarisation 0 PSF
        if float(psf_taylor[0, 0].max()):
            log.info("mmclean_kernel_list %s: Processing pol %d", prefix, pol)
            comp_array[:, pol], residual_array[:, pol] = msmfsclean(
                dirty_taylor[:, pol], psf_taylor[:, 0],
                None if window_taylor is None else window_taylor[0, pol],
                None if sensitivity_taylor is None else sensitivity_taylor[:, pol],
                gain, thresh, niter, scales, fracthresh, findpeak, prefix)
        else:
            log.info("mmclean_kernel_list %s: Skipping pol %d", prefix, pol)

    comp_taylor = _image_like(comp_array, moment_image)
    residual_taylor = _image_like(residual_array, moment_image)
    return (calculate_image_list_from_frequency_taylor_terms(dirty_list, comp_taylor),
            calculate_image_list_from_frequency_taylor_terms(dirty_list, residual_taylor))


def deconvolve_cube(dirty, psf, sensitivity=None, prefix="", **kwargs):
    """Clean an image cube, every channel and polarisation separately.

    For example::

        comp, residual = deconvolve_cube(dirty, psf, niter=1000, gain=0.7,
                                         algorithm="msclean", scales=[0, 3, 10, 30],
                                         threshold=0.01)

    :param dirty: dirty Image [nchan, npol, ny, nx]
    :param psf: PSF Image
    :param sensitivity: accepted and, as in the reference, not used: there it is
        handed on under a keyword that ``deconvolve_list`` does not read, so it
        never reaches the cleaner.  ``deconvolve_list(sensitivity_list=...)``
        does use it.
    :param kwargs: see ``deconvolve_list``
    :return: component Image, residual Image
    """
    dirty_list = _scatter_channels(dirty)
    psf_list = _scatter_channels(psf)
    comp_list, residual_list = deconvolve_list(dirty_list, psf_list, prefix=prefix, **kwargs)
    return _gather_channels(comp_list), _gather_channels(residual_list)


# ---- restore ---------------------------------------------------------------
def _gaussian_coefficients(x_stddev, y_stddev, theta):
    """a, b, c of exp(-(a dx^2 + b dx dy + c dy^2)) for a rotated Gaussian."""
    cos2, sin2, s2t = math.cos(theta) ** 2, math.sin(theta) ** 2, math.sin(2.0 * theta)
    xs2, ys2 = x_stddev ** 2, y_stddev ** 2
    return (0.5 * (cos2 / xs2 + sin2 / ys2), 0.5 * (s2t / xs2 - s2t / ys2),
            0.5 * (sin2 / xs2 + cos2 / ys2))


def _gaussian_kernel(x_stddev, y_stddev, theta):
    """Peak-normalised elliptical Gaussian sampled at pixel centres on a square
    box of side ceil(8 * max stddev) rounded up to odd (host, float64)."""
    size = int(math.ceil(8.0 * max(x_stddev, y_stddev)))
    size += 1 - size % 2
    a, b, c = _gaussian_coefficients(x_stddev, y_stddev, theta)
    d = numpy.arange(size, dtype=float) - size // 2
    dy, dx = numpy.meshgrid(d, d, indexing="ij")
    kernel = numpy.exp(-(a * dx**2 + b * dx * dy + c * dy**2))
    return kernel / kernel.max()


def _convolve_wrap(planes, kernel):
    """Circular convolution of device planes [..., ny, nx] with a centred odd kernel."""
    ny, nx = planes.shape[-2:]
    k = kernel.shape[0]
    if k > ny or k > nx:
        raise ValueError(f"restore: the {k} x {k} clean-beam box exceeds the {ny} x {nx} image")
    padded = torch.zeros((ny, nx), dtype=torch.float64, device=planes.device)
    padded[:k, :k] = torch.as_tensor(kernel, device=planes.device)
    padded = torch.roll(padded, (-(k // 2), -(k // 2)), dims=(0, 1))
    return torch.fft.ifft2(torch.fft.fft2(planes) * torch.fft.fft2(padded)).real


def restore_list(model_list, psf_list=None, residual_list=None, clean_beam=None):
    """Restore: each model plane convolved (circularly, on the device) with the
    peak-normalised clean beam, plus the residual.

    :param model_list: list of model Images
    :param psf_list: list of PSF Images, fitted for the beam when ``clean_beam`` is None
    :param residual_list: list of residual Images, or None
    :param clean_beam: {"bmaj", "bmin", "bpa"} in (deg, deg, deg)
    :return: list of restored Images, ``attrs["clean_beam"]`` set
    """
    restored_list = []
    for channel, model in enumerate(model_list):
        psf = psf_list[channel] if psf_list is not None else None
        residual = residual_list[channel] if residual_list is not None else None
        if clean_beam is None:
            if psf is None:
                raise ValueError("restore_list: Either the psf or the clean_beam must be specified")
            clean_beam = fit_psf(psf)
            log.info("restore_list: Using fitted clean beam (deg, deg, deg) = %s", clean_beam)
        beam_pixels = convert_clean_beam_to_pixels(model, clean_beam)
        kernel = _gaussian_kernel(float(beam_pixels[0]), float(beam_pixels[1]), float(beam_pixels[2]))
        data = _convolve_wrap(_device.to_dev(_pixels(model), torch.float64), kernel)
        if residual is not None:
            data = data + _device.to_dev(_pixels(residual), torch.float64)
        restored = model.copy(deep=True, data=_device.like_input(data, _pixels(model)))
        restored.attrs["clean_beam"] = clean_beam
        restored_list.append(restored)
    return restored_list


def fit_psf(psf):
    """Fit an elliptical Gaussian to the central 15 x 15 pixels of plane [0, 0]
    of a PSF (least squares on the host, from unit widths and zero angle).

    :return: {"bmaj", "bmin", "bpa"} in (deg, deg, deg); a failed fit or a
        non-positive width gives the beam of 1-pixel standard deviation
    """
    from scipy.optimize import least_squares

    data = _pixels(psf)
    npixel = data.shape[3]
    sl = slice(npixel // 2 - 7, npixel // 2 + 8)
    z = data[0, 0, sl, sl]
    z = z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else numpy.asarray(z)
    z = z.astype(float)
    y, x = numpy.mgrid[sl, sl]
    if z.shape != x.shape:
        raise ValueError("fit_psf: the PSF is smaller than the 15 x 15 fitting box")

    def misfit(q):
        amp, x0, y0, xs, ys, theta = q
        a, b, c = _gaussian_coefficients(xs, ys, theta)
        dx, dy = x - x0, y - y0
        return (amp * numpy.exp(-(a * dx**2 + b * dx * dy + c * dy**2)) - z).ravel()

    try:
        with numpy.errstate(all="ignore"):
            fit = least_squares(misfit, [numpy.max(z), numpy.mean(x), numpy.mean(y), 1.0, 1.0, 0.0],
                                method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        if not numpy.all(numpy.isfinite(fit.x)) or fit.x[3] <= 0.0 or fit.x[4] <= 0.0:
            log.warning("fit_psf: error in fitting to psf, using 1 pixel stddev")
            beam_pixels = (1.0, 1.0, 0.0)
        else:
            beam_pixels = (float(fit.x[3]), float(fit.x[4]), float(fit.x[5]))
    except ValueError:
        log.warning("fit_psf: warning in fit to psf, using 1 pixel stddev")
        beam_pixels = (1.0, 1.0, 0.0)
    return convert_clean_beam_to_degrees(psf, beam_pixels)


def restore_cube(model, psf=None, residual=None, clean_beam=None):
    """Restore the model image to the residuals (see ``restore_list``).

    :param model: model Image (the clean components)
    :param psf: PSF Image, fitted for the beam when ``clean_beam`` is None
    :param residual: residual Image or None
    :param clean_beam: {"bmaj", "bmin", "bpa"} in (deg, deg, deg)
    :return: restored Image
    """
    restored_list = restore_list(model_list=_scatter_channels(model),
                                 psf_list=_scatter_channels(psf),
                                 residual_list=_scatter_channels(residual), clean_beam=clean_beam)
    restored = _gather_channels(restored_list)
    restored.attrs["clean_beam"] = restored_list[0].attrs["clean_beam"]
    return restored
