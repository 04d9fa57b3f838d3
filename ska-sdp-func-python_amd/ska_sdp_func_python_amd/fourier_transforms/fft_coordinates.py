"""Coordinates for centred FFTs, the spheroidal function and the w beam
(reference src/ska_sdp_func_python/fourier_transforms/fft_coordinates.py).

Host functions over numpy, with the reference's arithmetic operation by
operation.  ``grdsf`` is the one in sky_component/operations.py.
"""

__all__ = [
    "coordinates",
    "grdsf",
    "w_beam",
]

import logging

import numpy

from ..sky_component.operations import grdsf

log = logging.getLogger("func-python-logger")


def coordinateBounds(npixel):
    """Lowest and highest coordinate of an ``npixel`` axis whose step is
    1 / npixel and whose pixel npixel // 2 lies on zero (the axis of a
    shifted FFT).

    :param npixel: Number of pixels
    :return: (low, high)
    """
    if npixel % 2 == 0:
        return -0.5, 0.5 * (npixel - 2) / npixel
    return -0.5 * (npixel - 1) / npixel, 0.5 * (npixel - 1) / npixel


def coordinates(npixel: int):
    """1-D array spanning [-.5, .5[ with 0 at position npixel // 2.

    :param npixel: Number of pixels
    :return: 1D array containing coordinates
    """
    return (numpy.arange(npixel) - npixel // 2) / npixel


def coordinates2(npixel: int):
    """The two grids (row coordinate, column coordinate) of
    ``coordinates(npixel)`` over an npixel x npixel array.

    :param npixel: Number of pixels
    :return: Grid (2D array) containing coordinates
    """
    return (numpy.mgrid[0:npixel, 0:npixel] - npixel // 2) / npixel


def coordinates2Offset(npixel: int, cx: int, cy: int, quadrant=False):
    """Two grids of coordinates with step 1 / npixel and zero at pixel
    (cy, cx); with ``quadrant`` only the first npixel // 2 + 1 pixels of each
    axis.  Used for A and w beams.

    :param npixel: Number of pixels
    :param cx: location of delay centre (default npixel // 2)
    :param cy: location of delay centre (default npixel // 2)
    :return: (row coordinates, column coordinates)
    """
    if cx is None:
        cx = npixel // 2
    if cy is None:
        cy = npixel // 2
    n = npixel // 2 + 1 if quadrant else npixel
    rows, cols = numpy.mgrid[0:n, 0:n]
    return (rows - cy) / npixel, (cols - cx) / npixel


def w_beam(npixel, field_of_view, w, cx=None, cy=None, remove_shift=False):
    """W beam: the Fresnel pattern exp(-2 pi i w (1 - sqrt(1 - r^2))) of a
    non-coplanar baseline over the field, zero where r^2 >= 1.  One quadrant
    is computed and reflected about its last row and column, as the reference
    does.

    :param npixel: Size of the grid in pixels
    :param field_of_view: Field of view
    :param w: Baseline distance to the projection plane
    :param cx: location of delay centre (default npixel // 2)
    :param cy: location of delay centre (default npixel // 2)
    :param remove_shift: Divide by the value at the delay centre
    :return: npixel x npixel array with the far field
    """
    if cx is None:
        cx = npixel // 2
    if cy is None:
        cy = npixel // 2
    ly, mx = coordinates2Offset(npixel, cx, cy, quadrant=True)
    r2 = field_of_view**2 * (ly**2 + mx**2)
    ph = -2 * numpy.pi * w * (1 - numpy.sqrt(1.0 - r2))
    outside = r2 >= 1.0
    ph[outside] = 0
    cp = numpy.exp(1j * ph)
    cp[outside] = 0 + 0j
    cp[r2 == 0] = 1.0 + 0j
    if remove_shift:
        cp /= cp[-1, -1]
    extra = npixel % 2 - 1
    return numpy.pad(cp, ((0, int(cx) + extra), (0, int(cy) + extra)), "reflect")
