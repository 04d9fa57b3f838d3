"""Iterators over the facets and the channels of an image (reference
src/ska_sdp_func_python/image/iterators.py): ``image_raster_iter`` (:66-190)
and ``image_channel_iter`` (:193-246).

Pixels may be numpy arrays or device tensors.  A sub-image is a view of its
parent's pixels (a numpy or a torch slice), so writing through it updates
the parent; its WCS is a deep copy with the reference pixel moved.

The raster (:123-151): facets of ``dx = nx // facets`` by ``dy = ny // facets``
pixels, ``sx = dx - 2 * overlap`` and ``sy = dy - 2 * overlap`` apart, facet
(fy, fx) starting at ``x = nx // 2 + sx * (fx - facets // 2) - overlap`` and
the same in y, in fy-major order.  The 1-D tapers (:22-53) are computed on
the host with the reference's arithmetic.

Deviations from the reference:

* the y origin is checked like the x origin (the reference checks x alone and
  fails later with a broadcast error);
* a step ``sx <= 0`` or ``sy <= 0`` (``2 * overlap >= dx``) raises ValueError
  (the reference then stacks every facet on one spot);
* device pixels that are neither float32 nor float64 raise ValueError;
* all facets are checked before the first is yielded, so a raster that leaves
  the image yields nothing (the reference yields the facets in front of the
  offending one first).
"""

import logging

import numpy
import torch

from ..datamodels import Image
from ..util.array_functions import tukey_filter

__all__ = ["image_channel_iter", "image_raster_iter"]

log = logging.getLogger("func-python-logger")


def _taper_linear(npixels, over):
    ramp = numpy.arange(0, over).astype(float) / float(over)
    taper1d = numpy.ones(npixels)
    taper1d[:over] = ramp
    taper1d[(npixels - over):npixels] = 1.0 - ramp
    return taper1d


def _taper_quadratic(npixels, over):
    ramp = numpy.arange(0, over).astype(float) / float(over)
    half = over // 2
    quadratic_ramp = numpy.ones(over)
    quadratic_ramp[0:half] = 2.0 * ramp[0:half] ** 2
    quadratic_ramp[half:] = 1 - 2.0 * ramp[half:0:-1] ** 2
    taper1d = numpy.ones(npixels)
    taper1d[:over] = quadratic_ramp
    taper1d[(npixels - over):npixels] = 1.0 - quadratic_ramp
    return taper1d


def _taper_tukey(npixels, over):
    r = 2 * over / npixels
    return numpy.array([tukey_filter(x, r) for x in numpy.arange(npixels) / float(npixels)])


def _taper_flat(npixels, over=None):
    return numpy.ones([npixels])


_TAPERS = {"linear": _taper_linear, "quadratic": _taper_quadratic, "tukey": _taper_tukey}


def taper_1d(taper, npixels, overlap):
    """The 1-D taper of a facet side of ``npixels`` (float64); an unknown name
    or None is flat."""
    return _TAPERS.get(taper, _taper_flat)(npixels, overlap)


def _pixels(im):
    return im["pixels"].data


def raster_geometry(im, facets, overlap):
    """(dy, dx, sy, sx, y0, x0) of the raster of ``image_raster_iter`` for
    ``facets`` > 1, with the reference's refusals and those listed above."""
    if not im.image_acc.is_canonical():
        raise ValueError("Image is not canonical")
    pixels = _pixels(im)
    if isinstance(pixels, torch.Tensor) and pixels.is_cuda and \
            pixels.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"Device pixels must be float32 or float64, not {pixels.dtype}")
    ny, nx = pixels.shape[2], pixels.shape[3]
    if facets > ny or facets > nx:
        raise ValueError("Cannot have more raster elements than pixels")
    if facets < 1:
        raise ValueError("Facets cannot be zero or less")
    if overlap < 0:
        raise ValueError("Overlap must be zero or greater")
    if facets == 1:
        return ny, nx, ny, nx, 0, 0
    if overlap >= (nx // facets) or overlap >= (ny // facets):
        raise ValueError(f"Overlap in facets is too large {nx}, {facets}, {overlap}")
    dx, dy = nx // facets, ny // facets
    sx, sy = dx - 2 * overlap, dy - 2 * overlap
    if sx <= 0 or sy <= 0:
        raise ValueError(f"Overlap in facets leaves no step between them {nx}, {ny}, {facets}, "
                         f"{overlap}")
    x0 = nx // 2 - sx * (facets // 2) - overlap
    y0 = ny // 2 - sy * (facets // 2) - overlap
    if x0 < 0 or x0 + sx * (facets - 1) + dx > nx:
        raise ValueError(f"overlap too large: starting point {x0}")
    if y0 < 0 or y0 + sy * (facets - 1) + dy > ny:
        raise ValueError(f"overlap too large: starting point {y0}")
    return dy, dx, sy, sx, y0, x0


def image_raster_iter(im, facets=1, overlap=0, taper="flat", make_flat=False):
    """Generator of the ``facets`` x ``facets`` sub-images of an image,
    optionally overlapping, each with its own WCS.

    To update the image in place::

         for r in image_raster_iter(im, facets=2):
             r["pixels"].data[...] = numpy.sqrt(r["pixels"].data[...])

    With ``make_flat`` and an overlap the generator yields new images instead,
    which hold the taper of a facet, ``outer(taper_y, taper_x)`` in the
    image's dtype and on its device: ``image_gather_facets`` weights the
    facets with them.  Some combinations of image size, facets and overlap
    are invalid and raise ValueError.

    :param im: Image
    :param facets: Number of image partitions on each axis
    :param overlap: Overlap in pixels
    :param taper: 'linear', 'quadratic' or 'tukey'; anything else is flat
    :param make_flat: Make the flat images
    :returns: Generator of images
    """
    dy, dx, sy, sx, y0, x0 = raster_geometry(im, facets, overlap)
    if facets == 1:
        yield im
        return
    pixels = _pixels(im)
    flat = None
    if overlap > 0 and make_flat:
        flat = numpy.outer(taper_1d(taper, dy, overlap), taper_1d(taper, dx, overlap))
    for fy in range(facets):
        y = y0 + sy * fy
        for fx in range(facets):
            x = x0 + sx * fx
            wcs = im.image_acc.wcs.deepcopy()
            wcs.wcs.crpix[0] -= x
            wcs.wcs.crpix[1] -= y
            data = pixels[..., y:y + dy, x:x + dx]
            if flat is None:
                yield Image.constructor(data=data, wcs=wcs,
                                        polarisation_frame=im.image_acc.polarisation_frame)
                continue
            if isinstance(data, torch.Tensor):
                weights = torch.as_tensor(flat, device=data.device).to(data.dtype)
                weights = weights.expand(data.shape).contiguous()
            else:
                weights = numpy.zeros_like(data)
                weights[..., :, :] = flat
            yield Image.constructor(data=weights, wcs=wcs, clean_beam=im.attrs.get("clean_beam"),
                                    polarisation_frame=im.image_acc.polarisation_frame)


def image_channel_iter(im, subimages=1):
    """Generator of ``subimages`` contiguous blocks of channels of an image,
    each a view with ``crpix[3]`` moved to its first channel.

    To update the image in place::

         for r in image_channel_iter(im, subimages=nchan):
             r["pixels"].data[...] = numpy.sqrt(r["pixels"].data[...])

    :param im: Image
    :param subimages: Number of subimages
    :returns: Generator of images
    """
    assert isinstance(im, Image), im
    assert im.image_acc.is_canonical()
    pixels = _pixels(im)
    nchan = pixels.shape[0]
    assert subimages <= nchan, f"More subimages {subimages} than channels {nchan}"
    step = nchan // subimages
    channels = list(range(0, nchan, step))
    assert len(channels) == subimages, \
        f"subimages {subimages} does not match length of channels {len(channels)}"
    for i, channel in enumerate(channels):
        channel_max = channels[i + 1] if i + 1 < len(channels) else nchan
        wcs = im.image_acc.wcs.deepcopy()
        wcs.wcs.crpix[3] -= channel
        yield Image.constructor(data=pixels[channel:channel_max, ...], wcs=wcs,
                                polarisation_frame=im.image_acc.polarisation_frame)
