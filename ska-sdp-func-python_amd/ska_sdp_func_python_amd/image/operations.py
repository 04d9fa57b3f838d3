"""Image operations (reference src/ska_sdp_func_python/image/operations.py):
the clean-beam unit conversions (:32-75) and the two pol-frame converters,
which live in ``image_operations`` and are re-exported here."""

import numpy

from ..image_operations import convert_polimage_to_stokes, convert_stokes_to_polimage

__all__ = ["convert_clean_beam_to_degrees", "convert_clean_beam_to_pixels",
           "convert_polimage_to_stokes", "convert_stokes_to_polimage"]

# FWHM of a Gaussian in units of its standard deviation
_TO_FWHM = numpy.sqrt(8.0 * numpy.log(2.0))


def _cellsize(im):
    """Cell size in radians, from the DEC axis of the image's WCS."""
    return numpy.deg2rad(im.image_acc.wcs.wcs.cdelt[1])


def convert_clean_beam_to_degrees(im, beam_pixels):
    """Beam (stddev, stddev, angle in rad) in pixels -> {"bmaj", "bmin", "bpa"}
    in (deg, deg, deg); the larger width becomes bmaj, and when that is the
    first one the position angle turns by 90 degrees."""
    cellsize = _cellsize(im)
    if beam_pixels[1] > beam_pixels[0]:
        return {"bmaj": numpy.rad2deg(beam_pixels[1] * cellsize * _TO_FWHM),
                "bmin": numpy.rad2deg(beam_pixels[0] * cellsize * _TO_FWHM),
                "bpa": numpy.rad2deg(beam_pixels[2])}
    return {"bmaj": numpy.rad2deg(beam_pixels[0] * cellsize * _TO_FWHM),
            "bmin": numpy.rad2deg(beam_pixels[1] * cellsize * _TO_FWHM),
            "bpa": numpy.rad2deg(beam_pixels[2]) + 90.0}


def convert_clean_beam_to_pixels(model, clean_beam):
    """{"bmaj", "bmin", "bpa"} in (deg, deg, deg) -> (stddev of bmin, stddev of
    bmaj, angle in rad) in pixels of ``model``."""
    cellsize = _cellsize(model)
    return (numpy.deg2rad(clean_beam["bmin"]) / (cellsize * _TO_FWHM),
            numpy.deg2rad(clean_beam["bmaj"]) / (cellsize * _TO_FWHM),
            numpy.deg2rad(clean_beam["bpa"]))
