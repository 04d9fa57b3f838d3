"""What a pipeline puts between its imaging calls (reference
src/ska_sdp_func_python/imaging/imaging_helpers.py):

    sum_invert_results   (:25-58)    weighted sum of (image, sumwt) pairs
    remove_sumwt         (:61-72)    the images of such pairs
    sum_predict_results  (:75-93)    sum of model visibilities
    threshold_list       (:96-150)   clean threshold from the residuals' peak

numpy pixels and visibilities are processed by numpy with the reference's own
operations in its order.  Device tensors stay on the device:

* ``sum_invert_results`` makes one call of ``kernels.sum_planes`` for the whole
  list -- every dirty image read once, the sum written once, the weights
  applied per [chan, pol] plane and the division by the summed weights (or the
  zeroing of a plane without weight) done on the way out.  ``sumwt`` is summed
  on the host as the reference sums it; only these small tables cross to the
  device.  float64 pixels give numpy's bits.
* ``sum_predict_results`` adds the list onto the first entry's ``vis`` with
  one call of the same kernel, in the element type and list order: numpy's
  bits for complex64 and complex128.
* ``threshold_list`` takes each image's peak with ``kernels.peak_abs``, which
  sums the channels on the fly and reads a facet view where it lies; the
  moment image is never made.

Deviations, on the device only:

* float32 pixels in ``sum_invert_results`` are accumulated in float64 and
  rounded once; numpy rounds the sum to float32 at every list entry.
* ``threshold_list(use_moment0=True)`` reports "NaNs present" from flags the
  kernel sets when an element it reads or a channel mean is NaN, as
  image/taylor_terms.py documents for calculate_image_frequency_moments: +inf
  and -inf in different pixels do not trip it, which ``isnan(sum(data))`` does.
* ``sum_predict_results`` compares all shapes before it adds anything; the
  reference has added the entries before a mismatching one when it raises.
"""

import logging

import numpy
import torch

from ..datamodels import Image
from ..image.taylor_terms import calculate_image_frequency_moments
from .base import normalise_sumwt

__all__ = ["remove_sumwt", "sum_invert_results", "sum_predict_results", "threshold_list"]

log = logging.getLogger("func-python-logger")


def _on_device(a):
    return isinstance(a, torch.Tensor) and a.is_cuda


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def sum_invert_results(image_list):
    """Sum a set of invert results with appropriate weighting.

    :param image_list: List of (image, sum of weights) pairs; image: Image,
        sumwt: ndarray [nchan, npol].  Entries after the first may be None.
    :return: Image, sum of weights.  A list of one gives a deep copy of its
        image and its sumwt itself, not normalised.
    """
    if len(image_list) == 1:
        im = image_list[0][0].copy(deep=True)
        sumwt = image_list[0][1]
        return im, sumwt

    first = image_list[0][0]
    first_pixels = first["pixels"].data
    sumwt = numpy.array(_host(image_list[0][1]))
    sumwt *= 0.0
    entries = [arg for arg in image_list if arg is not None]

    if _on_device(first_pixels):
        from .. import kernels
        if not all(_on_device(arg[0]["pixels"].data) for arg in entries):
            raise ValueError("sum_invert_results: the images must all be on the device or all numpy")
        weights = numpy.stack([numpy.asarray(_host(arg[1]), dtype=numpy.float64) for arg in entries])
        if weights.shape[1:] != tuple(first_pixels.shape[:2]):
            raise ValueError(f"sum_invert_results: sumwt must be {tuple(first_pixels.shape[:2])}, "
                             f"not {weights.shape[1:]}")
        for arg in entries:
            sumwt += _host(arg[1])
        data = kernels.sum_planes([arg[0]["pixels"].data for arg in entries], weights, sumwt,
                                  normalise=True)
        im = Image.constructor(data=data, polarisation_frame=first.image_acc.polarisation_frame,
                               wcs=first.image_acc.wcs, clean_beam=first.attrs["clean_beam"])
        return im, sumwt

    im = Image.constructor(data=numpy.zeros_like(first_pixels),
                           polarisation_frame=first.image_acc.polarisation_frame,
                           wcs=first.image_acc.wcs, clean_beam=first.attrs["clean_beam"])
    for arg in entries:
        im["pixels"].data += arg[1][..., numpy.newaxis, numpy.newaxis] * arg[0]["pixels"].data
        sumwt += arg[1]
    im = normalise_sumwt(im, sumwt)
    return im, sumwt


def remove_sumwt(results):
    """Remove the sumwt term in a list of (image, sumwt) tuples.

    :param results: List of tuples (image, sumwt)
    :return: A list of just the images
    """
    try:
        return [d[0] for d in results]
    except KeyError:
        return results


def sum_predict_results(results):
    """Sum a set of predict results of the same shape.

    :param results: List of Visibilities to be summed; entries may be None
    :return: The first Visibility that is not None, summed in place
    """
    entries = [r for r in results if r is not None]
    if not entries:
        return None
    sum_results = entries[0]
    if _on_device(sum_results["vis"].data):
        from .. import kernels
        vis = [r["vis"].data for r in entries]
        for v in vis[1:]:
            assert vis[0].shape == v.shape
        if len(vis) > 1:
            if not all(_on_device(v) for v in vis):
                raise ValueError("sum_predict_results: the visibilities must all be on the device "
                                 "or all numpy")
            if vis[0].is_contiguous():
                kernels.sum_planes(vis, out=vis[0])
            else:
                vis[0].copy_(kernels.sum_planes(vis))
        return sum_results
    for result in entries[1:]:
        assert sum_results["vis"].data.shape == result["vis"].data.shape
        sum_results["vis"].data += result["vis"].data
    return sum_results


def _moment0_peak_device(im):
    """max |moment 0 / nchan| with the assertions of
    calculate_image_frequency_moments(im), the moment image never made."""
    from .. import kernels
    assert isinstance(im, Image), im
    assert im.image_acc.is_canonical()
    peak, flags = kernels.peak_abs(im["pixels"].data, "moment0")
    assert not flags & kernels.PEAK_NAN_INPUT, "NaNs present in image data"
    assert not flags, "NaNs present in moment data"
    return numpy.float64(peak)


def threshold_list(imagelist, threshold, fractional_threshold, use_moment0=True, prefix=""):
    """Find the actual clean threshold for a list of results, optionally from
    the peak of moment 0.

    :param imagelist: List of Images (sub-images may be views of a larger one)
    :param threshold: Absolute threshold
    :param fractional_threshold: Fractional threshold
    :param use_moment0: Use moment 0 (the channel mean) instead of the middle channel
    :param prefix: Prefix for logging information
    :return: Actual threshold
    """
    peak = 0.0
    for i, result in enumerate(imagelist):
        pixels = result["pixels"].data
        if use_moment0:
            if _on_device(pixels):
                this_peak = _moment0_peak_device(result)
            else:
                moments = calculate_image_frequency_moments(result)
                this_peak = numpy.max(numpy.abs(moments["pixels"].data[0, ...] / pixels.shape[0]))
            peak = max(peak, this_peak)
            log.info("threshold_list: using moment 0, sub_image %s, peak = %s", i, this_peak)
        else:
            ref_chan = pixels.shape[0] // 2
            if _on_device(pixels):
                from .. import kernels
                this_peak = numpy.float64(kernels.peak_abs(pixels, "refchan")[0])
            else:
                this_peak = numpy.max(numpy.abs(pixels[ref_chan]))
            peak = max(peak, this_peak)
            log.info("threshold_list: using refchan %s, sub_image %s, peak = %s", ref_chan, i,
                     this_peak)

    actual = max(peak * fractional_threshold, threshold)

    if use_moment0:
        log.info("threshold_list %s: Global peak in moment 0 = %s, sub-image clean threshold "
                 "will be %s", prefix, peak, actual)
    else:
        log.info("threshold_list %s: Global peak = %s, sub-image clean threshold will be %s",
                 prefix, peak, actual)
    return actual
