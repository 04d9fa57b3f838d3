"""Scatter of an image into facets or channels and the gathers that undo
them (reference src/ska_sdp_func_python/image/gather_scatter.py):
``image_scatter_facets`` / ``image_gather_facets`` (:24-166) over the raster
of ``iterators.image_raster_iter``, ``image_scatter_channels`` /
``image_gather_channels`` (:169-194).

Pixels may be numpy arrays or device tensors.  Scatter costs nothing: the
sub-images are views.  ``image_gather_facets`` has two paths with the same
bits: numpy pixels go through the reference's operations in the reference's
order; device pixels go through one call of ``kernels.gather_facets``
(csrc/facets.hip), which reads every facet pixel once and writes every output
pixel once -- no flats, no summed-flats image, no masked passes.  Either way
the result is a new image and ``im`` is only a template.

Deviations from the reference (see also ``iterators``):

* the facets given to ``image_gather_facets`` must agree with ``im`` in dtype
  and device and be [nchan, npol, dy, dx]; a list shorter than the raster
  raises ValueError (the reference broadcasts or fails inside numpy);
* ``image_scatter_channels(im, subimages=None)`` gives one image per channel;
  an integer must divide the number of channels and gives contiguous equal
  blocks, which is what xarray's equal-width ``groupby_bins`` gives for evenly
  spaced channels; any other integer raises ValueError.  Each block's WCS has
  ``crval[3]`` moved to its first channel;
* ``image_gather_channels`` concatenates the pixels along frequency and keeps
  the first image's WCS and attributes.
"""

import logging

import numpy
import torch

from ..datamodels import Image
from .iterators import image_raster_iter, raster_geometry, taper_1d

__all__ = ["image_gather_channels", "image_gather_facets", "image_scatter_channels",
           "image_scatter_facets"]

log = logging.getLogger("func-python-logger")


def _pixels(im):
    return im["pixels"].data


def _image_like(data, im):
    return Image.constructor(data=data, polarisation_frame=im.image_acc.polarisation_frame,
                             wcs=im.image_acc.wcs, clean_beam=im.attrs.get("clean_beam"))


def image_scatter_facets(im, facets=1, overlap=0, taper=None):
    """Scatter an image into a list of ``facets`` x ``facets`` sub-images
    (views) with ``image_raster_iter``.

    :param im: Image
    :param facets: Number of image partitions on each axis
    :param overlap: Number of pixels overlap
    :param taper: Taper at edges (not used by the scatter)
    :return: list of subimages
    """
    if im is None:
        return None
    return list(image_raster_iter(im, facets=facets, overlap=overlap, taper=taper))


def _check_facets(image_list, pixels, facets, dy, dx):
    count = facets * facets
    if len(image_list) < count:
        raise ValueError(f"{len(image_list)} facets given for a raster of {facets} x {facets}")
    planes = [_pixels(sub) for sub in image_list[:count]]
    shape = tuple(pixels.shape[:2]) + (dy, dx)
    for p in planes:
        if type(p) is not type(pixels) or p.dtype != pixels.dtype or \
                getattr(p, "device", None) != getattr(pixels, "device", None):
            raise ValueError("The facets must agree with the image in dtype and device")
        if tuple(p.shape) != shape:
            raise ValueError(f"A facet of shape {tuple(p.shape)} where {shape} is expected")
    return planes


def _gather_facets_numpy(planes, pixels, geometry, facets, overlap, taper, return_flat):
    """The reference's operations in the reference's order (:84-166)."""
    dy, dx, sy, sx, y0, x0 = geometry
    out = numpy.zeros_like(pixels)
    if overlap <= 0:
        if return_flat:
            out[...] = 1.0
            return out
        for f, plane in enumerate(planes):
            y, x = y0 + sy * (f // facets), x0 + sx * (f % facets)
            out[..., y:y + dy, x:x + dx] += plane[...]
        return out
    # every facet has the same flat: ones for a single facet (the iterator
    # then yields the image of ones itself), the taper's outer product else
    flat = numpy.ones(pixels.shape[:2] + (dy, dx), dtype=pixels.dtype)
    if facets > 1:
        flat[..., :, :] = numpy.outer(taper_1d(taper, dy, overlap), taper_1d(taper, dx, overlap))
    sum_flats = numpy.zeros_like(pixels)
    for f in range(facets * facets):
        y, x = y0 + sy * (f // facets), x0 + sx * (f % facets)
        if not return_flat:
            out[..., y:y + dy, x:x + dx] += flat * planes[f][...]
        sum_flats[..., y:y + dy, x:x + dx] += flat[...]
    if return_flat:
        return sum_flats
    out[sum_flats > 0.0] /= sum_flats[sum_flats > 0.0]
    out[sum_flats <= 0.0] = 0.0
    return out


def _gather_facets_device(planes, pixels, geometry, facets, overlap, taper, return_flat):
    from .. import kernels
    dy, dx, sy, sx, y0, x0 = geometry
    taper_y = taper_x = None
    if overlap > 0 and facets > 1:
        taper_y, taper_x = taper_1d(taper, dy, overlap), taper_1d(taper, dx, overlap)
        if (taper_y == 1.0).all() and (taper_x == 1.0).all():
            taper_y = taper_x = None  # weights of 1 need no table
    ny, nx = pixels.shape[2:]
    if return_flat:
        return kernels.gather_facet_weights(facets, pixels.shape[:2], (dy, dx), (ny, nx), (y0, x0),
                                            (sy, sx), pixels.dtype, pixels.device, taper_y, taper_x,
                                            normalise=overlap > 0)
    ready = []
    for p in planes:
        # a slice of a contiguous image has all the kernel asks for
        even = p.stride(3) == 1 and (p.shape[0] == 1 or p.shape[1] == 1 or
                                     p.stride(0) == p.stride(1) * p.shape[1])
        ready.append(p if even else p.contiguous())
    return kernels.gather_facets(ready, facets, (ny, nx), (y0, x0), (sy, sx), taper_y, taper_x,
                                 normalise=overlap > 0)


def image_gather_facets(image_list, im, facets=1, overlap=0, taper=None, return_flat=False):
    """Gather a list of sub-images back into an image: the inverse of
    ``image_scatter_facets``.  Where facets overlap, each is weighted with the
    taper of ``image_raster_iter(..., make_flat=True)`` and the sum is divided
    by the summed weights; a pixel that no facet covers is 0.

    :param image_list: List of subimages [nchan, npol, dy, dx] in fy-major order
    :param im: Template of the output Image (not written)
    :param facets: Number of image partitions on each axis
    :param overlap: Overlap between neighbours in pixels
    :param taper: 'linear', 'quadratic' or 'tukey'; anything else is flat
    :param return_flat: Return the summed weights (ones without an overlap)
        instead of the image
    :return: new Image with the WCS of ``im``
    """
    geometry = raster_geometry(im, facets, overlap)
    pixels = _pixels(im)
    planes = None
    if not return_flat:
        planes = _check_facets(list(image_list), pixels, facets, geometry[0], geometry[1])
    if isinstance(pixels, torch.Tensor):
        if not pixels.is_cuda:
            raise ValueError("Image pixels must be a numpy array or a device tensor")
        data = _gather_facets_device(planes, pixels, geometry, facets, overlap, taper, return_flat)
    else:
        data = _gather_facets_numpy(planes, pixels, geometry, facets, overlap, taper, return_flat)
    return _image_like(data, im)


def image_scatter_channels(im, subimages=None):
    """Scatter an image into a list of sub-images (views) along frequency.

    :param im: Image
    :param subimages: Number of equal blocks of channels, which must divide
        the number of channels; None for one image per channel
    :return: list of subimages
    """
    if im is None:
        return None
    pixels = _pixels(im)
    nchan = pixels.shape[0]
    if subimages is None:
        subimages = nchan
    if subimages < 1 or nchan % subimages != 0:
        raise ValueError(f"subimages {subimages} does not divide the {nchan} channels")
    width = nchan // subimages
    out = []
    for chan in range(0, nchan, width):
        wcs = im.image_acc.wcs.deepcopy()
        wcs.wcs.crval[3] += chan * wcs.wcs.cdelt[3]
        out.append(Image.constructor(data=pixels[chan:chan + width], wcs=wcs,
                                     polarisation_frame=im.image_acc.polarisation_frame))
    return out


def image_gather_channels(image_list):
    """Gather a list of sub-images back into an image along frequency.

    :param image_list: List of subimages
    :return: Image with the first sub-image's WCS and attributes
    """
    planes = [_pixels(im) for im in image_list]
    data = torch.cat(planes) if isinstance(planes[0], torch.Tensor) else numpy.concatenate(planes)
    first = image_list[0]
    out = Image.constructor(data=data, polarisation_frame=first.image_acc.polarisation_frame,
                            wcs=first.image_acc.wcs)
    for key, value in first.attrs.items():
        if key not in out.attrs or out.attrs[key] is None:
            out.attrs[key] = value
    return out
