"""Frequency Taylor terms of image lists (reference
src/ska_sdp_func_python/image/taylor_terms.py:160-288): the moments
sum_chan w_k(chan) * image[chan] with

    w_k = ((nu - nu_ref) / nu_ref) ** k,

and the channel images rebuilt from such moments.  ``mmclean_kernel_list``
forms the dirty and PSF moments with the first and turns the cleaned moments
back into per-channel lists with the second.

The weights are numpy on the host, the channel frequency comes from the
spectral axis of each image's WCS, and the channels are summed in ascending
order, as in the reference.  numpy pixels give numpy pixels, device tensors
give device tensors.
"""

import logging

import numpy
import torch

from ..datamodels import Image

__all__ = ["calculate_image_list_frequency_moments",
           "calculate_image_list_from_frequency_taylor_terms"]

log = logging.getLogger("func-python-logger")


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

    moment_data = _zeros([nmoment, npol, ny, nx], first)
    for moment in range(nmoment):
        for chan, im in enumerate(im_list):
            weight = numpy.power((freq[chan] - reference_frequency) / reference_frequency, moment)
            moment_data[moment] += im["pixels"].data[0] * float(weight[0])

    moment_wcs = im_list[0].image_acc.wcs.deepcopy()
    moment_wcs.wcs.ctype[3] = "MOMENT"
    moment_wcs.wcs.crval[3] = 0.0
    moment_wcs.wcs.crpix[3] = 1.0
    moment_wcs.wcs.cdelt[3] = 1.0
    moment_wcs.wcs.cunit[3] = ""
    return Image.constructor(data=moment_data,
                             polarisation_frame=im_list[0].image_acc.polarisation_frame,
                             wcs=moment_wcs)


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

    newims = []
    for chan in range(nchan):
        newim_data = _zeros(im_list[chan]["pixels"].data.shape, moments)
        for moment in range(nmoment):
            weight = numpy.power((frequency[chan] - reference_frequency) / reference_frequency,
                                 moment)
            newim_data[0] += moments[moment] * float(weight)
        newims.append(Image.constructor(
            data=newim_data, polarisation_frame=im_list[chan].image_acc.polarisation_frame,
            wcs=im_list[chan].image_acc.wcs))
    return newims
