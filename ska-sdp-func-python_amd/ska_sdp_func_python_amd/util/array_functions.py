"""Small array functions (reference src/ska_sdp_func_python/util/array_functions.py)."""

import numpy

__all__ = ["tukey_filter"]


def tukey_filter(x, r):
    """The Tukey (tapered cosine) window at ``x`` in [0, 1] with transition
    width ``r`` (reference :85-99): a half cosine over the first and the last
    ``r / 2``, 1 between them and outside [0, 1].

    :param x: coordinate (float)
    :param r: transition point of the filter (float)
    :returns: value of the filter at x
    """
    half = r / 2.0
    if 0.0 <= x < half:
        return 0.5 * (1.0 + numpy.cos(2.0 * numpy.pi * (x - half) / r))
    if 1 - half <= x <= 1.0:
        return 0.5 * (1.0 + numpy.cos(2.0 * numpy.pi * (x - 1 + half) / r))
    return 1.0
