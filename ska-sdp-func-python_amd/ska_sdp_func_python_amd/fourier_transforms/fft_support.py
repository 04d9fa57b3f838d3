"""Centred FFTs, padding and extraction (reference
src/ska_sdp_func_python/fourier_transforms/fft_support.py).

numpy in, numpy out with the reference's bits (its branch without pyfftw); a
torch tensor goes through torch.fft and slicing and stays where it lies, so a
device tensor is transformed by rocFFT.  Which axes are shifted follows the
reference case by case:

* 4 axes: shift and transform the last two;
* 5 axes: ``fft`` shifts and transforms the last two, ``ifft`` shifts the
  last *three* and transforms the last two (the reference's own quirk);
* anything else: shift every axis, transform the last two.
"""

__all__ = [
    "extract_mid",
    "extract_oversampled",
    "fft",
    "ifft",
    "pad_mid",
]

import numpy
import torch


def _shift_axes(ndim, inverse):
    if ndim == 4:
        return [2, 3]
    if ndim == 5:
        return [2, 3, 4] if inverse else [3, 4]
    return None


def _centred(a, inverse):
    axes = _shift_axes(len(a.shape), inverse)
    if isinstance(a, torch.Tensor):
        dim = None if axes is None else tuple(axes)
        x = torch.fft.ifftshift(a, dim=dim)
        x = torch.fft.ifft2(x) if inverse else torch.fft.fft2(x)
        return torch.fft.fftshift(x, dim=dim)
    x = numpy.fft.ifftshift(a, axes=axes)
    x = numpy.fft.ifft2(x) if inverse else numpy.fft.fft2(x)
    return numpy.fft.fftshift(x, axes=axes)


def fft(a):
    """Fourier transformation from image to grid space, zero frequency and
    zero position both at pixel n // 2.

    :param a: image in `lm` coordinate space
    :return: `uv` grid
    """
    return _centred(a, False)


def ifft(a):
    """Fourier transformation from grid to image space, zero frequency and
    zero position both at pixel n // 2.

    :param a: `uv` grid to transform
    :return: an image in `lm` coordinate space
    """
    return _centred(a, True)


def pad_mid(ff, npixel):
    """Pad a far field with zeroes to ``npixel`` x ``npixel`` (the two
    innermost axes), keeping its centre nx // 2 at npixel // 2.  ``ff`` itself
    comes back when it has that size already.  As in the reference, an odd
    size is not handled properly.

    :param ff: The input far field, smaller than npixel x npixel
    :param npixel: The desired far field size
    :return: Padded array
    """
    ny, nx = ff.shape[-2:]
    if npixel == nx:
        return ff
    assert npixel > nx and npixel > ny
    py = npixel // 2 - ny // 2
    px = npixel // 2 - nx // 2
    if isinstance(ff, torch.Tensor):
        return torch.nn.functional.pad(ff, (px, px, py, py), mode="constant", value=0.0)
    width = [(0, 0)] * (ff.ndim - 2) + [(py, py), (px, px)]
    return numpy.pad(ff, pad_width=width, mode="constant", constant_values=0.0)


def extract_mid(a, npixel):
    """The ``npixel`` x ``npixel`` section about the centre of the two
    innermost axes: the reverse of ``pad_mid``.  As in the reference, the row
    slice is taken about the centre of the *last* axis and the column slice
    about the centre of the one before it.

    :param a: grid from which to extract
    :param npixel: desired size of the section to extract
    :return: Section of grid
    """
    ny, nx = a.shape[-2:]
    cx = nx // 2
    cy = ny // 2
    s = npixel // 2
    odd = npixel % 2
    return a[..., cx - s:cx + s + odd, cy - s:cy + s + odd]


def extract_oversampled(a, xf, yf, kernel_oversampling, kernelwidth):
    """The (xf, yf)-th kernel of an oversampled parent: every
    ``kernel_oversampling``-th pixel from ``kernelwidth // 2`` kernel pixels
    before the centre less the offset, times ``kernel_oversampling`` squared.
    An offset of (xf, yf) is the kernel for a sub-grid offset of (-xf, -yf).

    :param a: grid from which to extract
    :param xf: Offset in x
    :param yf: Offset in y
    :param kernel_oversampling: oversampling factor
    :param kernelwidth: size of section
    """
    assert 0 <= xf < kernel_oversampling
    assert 0 <= yf < kernel_oversampling
    centre = a.shape[0] // 2
    step = kernel_oversampling
    my = centre - step * (kernelwidth // 2) - yf
    mx = centre - step * (kernelwidth // 2) - xf
    assert mx >= 0 and my >= 0, f"mx {mx} and my {my}"
    mid = a[my:my + step * kernelwidth:step, mx:mx + step * kernelwidth:step]
    # os * os first: (mid * os) * os rounds differently when os is no power of two
    return step * step * mid
