"""Frequency Taylor terms of image cubes and image lists (reference
src/ska_sdp_func_python/image/taylor_terms.py): the moments
sum_chan w_k(chan) * image[chan] with

    w_k = ((nu - nu_ref) / nu_ref) ** k,

the channel images rebuilt from such moments, and the decoupled Taylor-term
images sum_chan pinv(coupling)[k, chan] * image[chan] that a continuum
pipeline writes out as its products.  ``mmclean_kernel_list`` forms the dirty
and PSF moments with the list form of the first and turns the cleaned moments
back into per-channel lists with the second.

    calculate_image_frequency_moments                  (:22-98)    cube
    calculate_image_from_frequency_taylor_terms        (:101-157)  cube
    calculate_image_list_frequency_moments             (:160-237)  list
    calculate_image_list_from_frequency_taylor_terms   (:240-288)  list
    calculate_frequency_taylor_terms_from_image_list   (:291-357)  list

All five are one operation, a small real matrix applied across a stack of
image planes.  The matrix -- the weights, and for the decoupled terms
``numpy.linalg.pinv(coupling, rcond=1e-7)`` -- is numpy on the host, the
channel frequencies come from the spectral axis of each image's WCS, and the
planes are summed in ascending order, as in the reference.  numpy pixels are
processed by numpy with the reference's own operations and give numpy pixels.
Device tensors stay on the device and give float64 device tensors: float64
and, in the three functions added with the kernel, float32 pixels go through
``kernels.mix_planes``, which reads every input plane once and writes every
output plane once and reproduces numpy's ``out[k] += in[c] * w`` bit for bit
(float32 pixels are promoted to float64 before the multiply, as numpy does
for the reference's float64 weights).  Device pixels of any other dtype in
the two list functions that predate the kernel keep their torch loop.

One deviation, on the device only: calculate_image_frequency_moments reports
"NaNs present" from a flag that the kernel sets when an element it reads or
writes is NaN.  The reference tests ``isnan(sum(data))``, which also fires
for +inf and -inf in different pixels of otherwise NaN-free data; the flag
does not, unless they meet in one output pixel.
"""

import logging

import numpy
import torch

from ..datamodels import Image

__all__ = ["calculate_image_frequency_moments",
           "calculate_image_from_frequency_taylor_terms",
           "calculate_image_list_frequency_moments",
           "calculate_image_list_from_frequency_taylor_terms",
           "calculate_frequency_taylor_terms_from_image_list"]

log = logging.getLogger("func-python-logger")


def _on_device(pixels):
    return isinstance(pixels, torch.Tensor) and pixels.is_cuda


def _mix(planes, weights, shape, check_nan=False):
    """kernels.mix_planes on the leading-axis planes of device pixels."""
    from .. import kernels
    out = torch.empty(tuple(shape), dtype=torch.float64, device=planes[0].device)
    flags = kernels.mix_planes([p.contiguous() for p in planes], weights, out,
                               check_nan=check_nan)
    return (out, flags[1]) if check_nan else out


def _moment_wcs(wcs):
    moment_wcs = wcs.deepcopy()
    moment_wcs.wcs.ctype[3] = "MOMENT"
    moment_wcs.wcs.crval[3] = 0.0
    moment_wcs.wcs.crpix[3] = 1.0
    moment_wcs.wcs.cdelt[3] = 1.0
    moment_wcs.wcs.cunit[3] = ""
    return moment_wcs


def _f64(pixels):
    """numpy pixels as float64 (float32 is promoted before the multiply)."""
    return numpy.asarray(pixels, dtype=numpy.float64)


def calculate_image_frequency_moments(im, reference_frequency=None, nmoment=1):
    """Frequency-weighted moments of an image cube.

    The spectral axis of the result is a MOMENT axis.

    :param im: Image cube [nchan, npol, ny, nx]
    :param reference_frequency: reference frequency (default: that of channel nchan // 2)
    :param nmoment: number of moments, 1 .. nchan
    :return: moments Image [nmoment, npol, ny, nx], float64
    """
    assert isinstance(im, Image), im
    assert im.image_acc.is_canonical()
    assert nmoment > 0
    pixels = im["pixels"].data
    nchan, npol, ny, nx = pixels.shape
    channels = numpy.arange(nchan)
    freq = im.image_acc.wcs.sub(["spectral"]).wcs_pix2world(channels, 0)[0]
    assert nmoment <= nchan, (f"Number of moments {nmoment} cannot exceed "
                              f"the number of channels {nchan}")
    if reference_frequency is None:
        reference_frequency = freq[nchan // 2]
    log.debug("calculate_image_frequency_moments: Reference frequency = %.3f (MHz)",
              reference_frequency / 1e6)

    weights = numpy.array([[numpy.power((freq[chan] - reference_frequency) / reference_frequency,
                                        moment) for chan in range(nchan)]
                           for moment in range(nmoment)])
    if _on_device(pixels) and pixels.dtype in (torch.float32, torch.float64):
        from .. import kernels
        moment_data, flags = _mix(list(pixels), weights, [nmoment, npol, ny, nx], check_nan=True)
        assert not flags & kernels.MIX_NAN_INPUT, "NaNs present in image data"
        assert not flags, "NaNs present in moment data"
    else:
        if isinstance(pixels, torch.Tensor):
            raise ValueError("device pixels must be float32 or float64; host pixels numpy")
        moment_data = numpy.zeros([nmoment, npol, ny, nx])
        assert not numpy.isnan(numpy.sum(pixels)), "NaNs present in image data"
        for moment in range(nmoment):
            for chan in range(nchan):
                moment_data[moment, ...] += _f64(pixels[chan, ...]) * weights[moment, chan]
        assert not numpy.isnan(numpy.sum(moment_data)), "NaNs present in moment data"

    return Image.constructor(data=moment_data,
                             polarisation_frame=im.image_acc.polarisation_frame,
                             wcs=_moment_wcs(im.image_acc.wcs))


def calculate_image_from_frequency_taylor_terms(im, taylor_terms_image, reference_frequency=None):
    """An image cube rebuilt from frequency Taylor terms:
    image[chan] = sum_k w_k(chan) * taylor_term[k].  A new Image is made.

    :param im: Image cube [nchan, npol, ny, nx] that gives the channels'
        frequencies, the WCS and the polarisation frame
    :param taylor_terms_image: Taylor-terms Image [nterms, npol, ny, nx]
    :param reference_frequency: reference frequency (default: that of channel nchan // 2)
    :return: rebuilt Image with ``im``'s WCS; numpy pixels have ``im``'s dtype as in
        the reference, device pixels are float64
    """
    nchan, npol, ny, nx = im["pixels"].data.shape
    terms = taylor_terms_image["pixels"].data
    n_taylor_terms, mnpol, mny, mnx = terms.shape
    if n_taylor_terms <= 0:
        raise ValueError("calculate_image_from_frequency_taylor_terms: "
                         "the number of taylor terms must be greater than zero")
    assert npol == mnpol
    assert ny == mny
    assert nx == mnx
    frequency = im.frequency.data
    if reference_frequency is None:
        reference_frequency = frequency[nchan // 2]
    log.debug("calculate_image_from_frequency_moments: Reference frequency = %.3f (MHz)",
              1e-6 * reference_frequency)

    weights = numpy.array([[numpy.power((frequency[chan] - reference_frequency)
                                        / reference_frequency, taylor_term)
                            for taylor_term in range(n_taylor_terms)] for chan in range(nchan)])
    if _on_device(terms) and terms.dtype in (torch.float32, torch.float64):
        newim_data = _mix(list(terms), weights, [nchan, npol, ny, nx])
    else:
        if isinstance(terms, torch.Tensor):
            raise ValueError("device pixels must be float32 or float64; host pixels numpy")
        newim_data = numpy.zeros_like(numpy.asarray(im["pixels"].values))
        for taylor_term in range(n_taylor_terms):
            for chan in range(nchan):
                newim_data[chan, ...] += _f64(terms[taylor_term, ...]) * weights[chan, taylor_term]
    return Image.constructor(data=newim_data,
                             polarisation_frame=im.image_acc.polarisation_frame,
                             wcs=im.image_acc.wcs)


def _zeros(shape, like):
    if isinstance(like, torch.Tensor):
        return torch.zeros(tuple(shape), dtype=torch.float64, device=like.device)
    return numpy.zeros(shape)


def _channel_frequencies(im_list):
    return [im.image_acc.wcs.sub(["spectral"]).wcs_pix2world([0], 0)[0] for im in im_list]


def calculate_image_list_frequency_moments(im_list, reference_frequency=None, nmoment=1):
    """Frequency-weighted moments of a list of single-channel images.

    The spectral axis of the result is a MOMENT axis.

    :param im_list: list of Images [1, npol, ny, nx]
    :param reference_frequency: reference frequency (default: that of channel nchan // 2)
    :param nmoment: number of moments, 1 .. nchan
    :return: moments Image [nmoment, npol, ny, nx], or None if ``im_list[0]`` is None
    """
    if nmoment <= 0:
        raise ValueError(f"Number of moments {nmoment} must be > 0")
    if im_list[0] is None:
        return None
    nchan = len(im_list)
    first = im_list[0]["pixels"].data
    _, npol, ny, nx = first.shape
    freq = _channel_frequencies(im_list)
    if nmoment > nchan:
        raise ValueError(f"Number of moments {nmoment} cannot exceed the number of channels {nchan}")
    if reference_frequency is None:
        reference_frequency = freq[nchan // 2]
    log.debug("calculate_image_frequency_moments: Reference frequency = %.3f (MHz)",
              float(numpy.ravel(reference_frequency)[0]) / 1e6)

    if _on_device(first) and all(im["pixels"].data.dtype == torch.float64 for im in im_list):
        weights = [[float(numpy.power((freq[chan] - reference_frequency) / reference_frequency,
                                      moment)[0]) for chan in range(nchan)]
                   for moment in range(nmoment)]
        moment_data = _mix([im["pixels"].data[0] for im in im_list], weights,
                           [nmoment, npol, ny, nx])
    else:
        moment_data = _zeros([nmoment, npol, ny, nx], first)
        for moment in range(nmoment):
            for chan, im in enumerate(im_list):
                weight = numpy.power((freq[chan] - reference_frequency) / reference_frequency,
                                     moment)
                moment_data[moment] += im["pixels"].data[0] * float(weight[0])

    return Image.constructor(data=moment_data,
                             polarisation_frame=im_list[0].image_acc.polarisation_frame,
                             wcs=_moment_wcs(im_list[0].image_acc.wcs))


def calculate_image_list_from_frequency_taylor_terms(im_list, moment_image, reference_frequency=None):
    """Channel images rebuilt from frequency moments (Taylor terms):
    image[chan] = sum_k w_k(chan) * moment[k].

    :param im_list: list of Images [1, npol, ny, nx] that give the channels'
        frequencies, WCS and polarisation frames
    :param moment_image: moments Image [nmoment, npol, ny, nx]
    :param reference_frequency: reference frequency (default: that of channel nchan // 2)
    :return: list of rebuilt Images
    """
    nchan = len(im_list)
    moments = moment_image["pixels"].data
    nmoment = moments.shape[0]
    frequency = numpy.array([d.frequency.data[0] for d in im_list])
    if reference_frequency is None:
        reference_frequency = frequency[nchan // 2]
    log.debug("calculate_image_from_frequency_moments: Reference frequency = %.3f (MHz)",
              1e-6 * reference_frequency)

    fused = None
    if _on_device(moments) and moments.dtype == torch.float64 and nchan > 0 and nmoment > 0 \
            and all(tuple(im["pixels"].data.shape) == (1,) + tuple(moments.shape[1:])
                    for im in im_list):
        weights = [[float(numpy.power((frequency[chan] - reference_frequency)
                                      / reference_frequency, moment))
                    for moment in range(nmoment)] for chan in range(nchan)]
        fused = _mix(list(moments), weights, (nchan, 1) + tuple(moments.shape[1:]))

    newims = []
    for chan in range(nchan):
        if fused is not None:
            newim_data = fused[chan]
        else:
            newim_data = _zeros(im_list[chan]["pixels"].data.shape, moments)
            for moment in range(nmoment):
                weight = numpy.power((frequency[chan] - reference_frequency)
                                     / reference_frequency, moment)
                newim_data[0] += moments[moment] * float(weight)
        newims.append(Image.constructor(
            data=newim_data, polarisation_frame=im_list[chan].image_acc.polarisation_frame,
            wcs=im_list[chan].image_acc.wcs))
    return newims


def calculate_frequency_taylor_terms_from_image_list(im_list, nmoment=1, reference_frequency=None):
    """Decoupled frequency Taylor-term images of a list of single-channel
    images: term[k] = sum_chan pinv(coupling)[k, chan] * image[chan], with
    coupling[chan, k] = w_k(chan) and the pseudo-inverse taken on the host
    (``numpy.linalg.pinv(coupling, rcond=1e-7)``).

    :param im_list: list of Images [1, npol, ny, nx]
    :param nmoment: number of Taylor terms
    :param reference_frequency: reference frequency (default: that of channel nchan // 2)
    :return: list of ``nmoment`` single-channel Images, float64, on a FREQ axis at the
        reference frequency
    """
    nchan = len(im_list)
    first = im_list[0]["pixels"].data
    single_chan, npol, ny, nx = first.shape
    if single_chan > 1:
        raise ValueError("calculate_frequency_taylor_terms_from_image_list: "
                         "each image must be single channel")
    frequency = numpy.array([d.frequency.data[0] for d in im_list])
    if reference_frequency is None:
        reference_frequency = frequency[len(frequency) // 2]
    log.debug("calculate_image_from_frequency_moments: Reference frequency = %.3f (MHz)",
              1e-6 * reference_frequency)

    wcs = im_list[nchan // 2].image_acc.wcs.deepcopy()
    wcs.wcs.ctype[3] = "FREQ"
    wcs.wcs.crval[3] = reference_frequency
    wcs.wcs.crpix[3] = 1.0
    wcs.wcs.cdelt[3] = 1.0
    wcs.wcs.cunit[3] = "Hz"
    polarisation_frame = im_list[nchan // 2].image_acc.polarisation_frame

    channel_moment_coupling = numpy.zeros([nchan, nmoment])
    for chan in range(nchan):
        for m in range(nmoment):
            channel_moment_coupling[chan, m] += numpy.power(
                (frequency[chan] - reference_frequency) / reference_frequency, m)
    pinv = numpy.linalg.pinv(channel_moment_coupling, rcond=1e-7)

    if _on_device(first) and first.dtype in (torch.float32, torch.float64):
        decoupled = _mix([im["pixels"].data[0] for im in im_list], pinv, [nmoment, 1, npol, ny, nx])
        decoupled_data_list = list(decoupled)
    else:
        if isinstance(first, torch.Tensor):
            raise ValueError("device pixels must be float32 or float64; host pixels numpy")
        decoupled_data_list = []
        for moment in range(nmoment):
            decoupled_data = numpy.zeros([1, npol, ny, nx])
            for chan in range(nchan):
                decoupled_data[0] += pinv[moment, chan] * _f64(im_list[chan]["pixels"].data[0, ...])
            decoupled_data_list.append(decoupled_data)
    return [Image.constructor(data=data, polarisation_frame=polarisation_frame, wcs=wcs)
            for data in decoupled_data_list]
