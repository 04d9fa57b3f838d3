"""Creation of the ``gcfcf`` that the AW-projection imagers and the
convolution-function gridder take: a grid-correction Image and an oversampled,
w-indexed ConvolutionFunction.

Neither function is in the reference, which grids with a convolution function
but cannot make one; they play the role of RASCIL's functions of the same
names and are defined by this recipe, written with the reference's
fourier_transforms (``os = oversampling``, ``h = os // 2``, ``nd = 2 h + 1``,
``N = farfield_npixel``, ``fov = nx * cell``, ``w_z = (z - nw // 2) * wstep``)::

    t   = grdsf(|2 * coordinates(N)|)[0]          (ones without use_aaf)
    A_z = w_beam(N, fov, -w_z) * outer(t, t) [* pb[chan, pol]]
    F_z = ifft(pad_mid(A_z, os * N))
    cf[chan, pol, z, iv, iu] = extract_oversampled(F_z, iu - h, iv - h, os, support)

with the slice arithmetic of extract_oversampled carried on to negative
offsets.  There are nd, not os, offset planes per axis because spatial_mapping
computes the offset index as round(delta * os) + h for delta in [-1/2, 1/2]:
with an even os both ends occur (they hold the same samples, one kernel pixel
apart).  The sign of w: the gridder adds conj(cf) and the image is the inverse
FFT of the grid, so cf has to be the inverse FFT of the conjugate of the screen
w_beam(w) that a visibility at w carries, and conj(w_beam(w)) = w_beam(-w).

The kernels are computed on the device by csrc/wkernel.hip, which evaluates
only the os * N-point transform's samples that the extraction reads and never
forms the padded plane.
"""

import numpy as np
import torch

from .. import _device, kernels
from ..datamodels import (WCS, ConvolutionFunction, Image, PolarisationFrame,
                          create_griddata_from_image)
from ..fourier_transforms.fft_coordinates import coordinates, grdsf

__all__ = ["create_awterm_convolutionfunction", "create_pswf_convolutionfunction"]


def default_farfield_npixel(support):
    """The smallest even number that is at least max(support + 2, 32)."""
    n = max(int(support) + 2, 32)
    return n + n % 2


def _frame(im, polarisation_frame):
    if polarisation_frame is None:
        return im.image_acc.polarisation_frame
    if isinstance(polarisation_frame, PolarisationFrame):
        return polarisation_frame
    return PolarisationFrame(polarisation_frame)


def cf_geometry(im, nw=1, wstep=1e15, oversampling=8, support=16, farfield_npixel=None, pb=None,
                polarisation_frame=None):
    """Check the arguments of create_awterm_convolutionfunction (ValueError
    for what it refuses; nothing here touches the device) and return what the
    recipe needs: a dict with nchan, npol, nx, N, os, h, nd, support, nw, fov
    (radians), the plane values w [nw] and the polarisation frame."""
    shape = tuple(im["pixels"].data.shape)
    if len(shape) != 4 or shape[2] != shape[3]:
        raise ValueError(f"the image must be [nchan, npol, n, n]: non-square {shape} is refused")
    iw = im.image_acc.wcs.wcs
    if abs(iw.cdelt[0]) != abs(iw.cdelt[1]):
        raise ValueError(f"the image's cells must be square: |cdelt| is {abs(iw.cdelt[0])} by "
                         f"{abs(iw.cdelt[1])}")
    support, oversampling, nw = int(support), int(oversampling), int(nw)
    if support < 2 or support % 2:
        raise ValueError(f"support {support} must be even and at least 2")
    if oversampling < 1:
        raise ValueError(f"oversampling {oversampling} must be at least 1")
    if nw < 1:
        raise ValueError(f"nw {nw} must be at least 1")
    n = default_farfield_npixel(support) if farfield_npixel is None else int(farfield_npixel)
    if n % 2 or n < support + 2:
        raise ValueError(f"farfield_npixel {n} must be even and at least support + 2 = "
                         f"{support + 2}")
    pf = _frame(im, polarisation_frame)
    nchan, nx = shape[0], shape[3]
    if pb is not None and tuple(pb.shape) != (nchan, pf.npol, n, n):
        raise ValueError(f"pb must be [nchan, npol, N, N] = {(nchan, pf.npol, n, n)}, not "
                         f"{tuple(pb.shape)}")
    cell = float(np.deg2rad(abs(iw.cdelt[1])))
    h = oversampling // 2
    return dict(nchan=nchan, npol=pf.npol, nx=nx, N=n, os=oversampling, h=h, nd=2 * h + 1,
                support=support, nw=nw, fov=nx * cell,
                w=[(z - nw // 2) * float(wstep) for z in range(nw)], frame=pf)


def cf_wcs_for_image(im, nw, wstep, oversampling, support):
    """The 7-axis WCS (u, v, du, dv, w, stokes, freq) of a convolution function
    for ``im``: the uv cell of create_griddata_from_image (signs included), the
    offset planes 1 / oversampling of it apart with offset 0 on plane h, w = 0
    on plane nw // 2."""
    gw = create_griddata_from_image(im).griddata_acc.griddata_wcs.wcs
    cdu, cdv = float(gw.cdelt[0]), float(gw.cdelt[1])
    h = oversampling // 2
    iw = im.image_acc.wcs.wcs
    return WCS(7, ["UU", "VV", "DUU", "DVV", "WW", "STOKES", "FREQ"],
               [support // 2 + 1, support // 2 + 1, h + 1, h + 1, nw // 2 + 1, 1, 1],
               [cdu, cdv, cdu / oversampling, cdv / oversampling, float(wstep), 1, float(iw.cdelt[3])],
               [0, 0, 0, 0, 0, 1, float(np.asarray(im.frequency.data)[0])])


def grid_correction_pixels(nchan, npol, nx, use_aaf=True):
    """The grid correction [nchan, npol, nx, nx], real float64 on the host:
    1 / (tg (x) tg) with tg = grdsf(|2 * coordinates(nx)|)[0], or ones."""
    if use_aaf:
        tg = grdsf(np.abs(2 * coordinates(nx)))[0]
        plane = 1 / np.outer(tg, tg)
    else:
        plane = np.ones((nx, nx))
    return np.broadcast_to(plane, (nchan, npol, nx, nx)).copy()


def create_awterm_convolutionfunction(im, nw=1, wstep=1e15, oversampling=8, support=16,
                                      use_aaf=True, farfield_npixel=None, pb=None,
                                      polarisation_frame=None, normalise=True):
    """Grid correction and oversampled w-projection (optionally AW)
    convolution function for imaging onto ``im``, computed on the device.  Not
    in the reference (see the module's text for the recipe that defines it);
    use the result as ``gcfcf=lambda _im: (gcf, cf)``.

    :param im: template Image, square with square cells; its pixels decide
        where the results live (numpy: host, device tensor: device)
    :param nw: number of w planes; plane z is at (z - nw // 2) * wstep
    :param wstep: distance of the w planes in wavelengths
    :param oversampling: sub-grid offsets per uv cell; the convolution
        function has 2 (oversampling // 2) + 1 offset planes per axis
    :param support: kernel width in uv cells (even)
    :param use_aaf: taper the far field with the spheroidal function (and
        correct for it in the grid correction)
    :param farfield_npixel: pixels N across the field on which the far field
        is sampled (even, at least support + 2; default: the smallest even
        number that is at least max(support + 2, 32))
    :param pb: optional primary beam [nchan, npol, N, N], real or complex,
        numpy or device tensor, in the image's pixel orientation, sampled on N
        points across the image's field with the centre at N // 2
    :param polarisation_frame: frame of the visibilities to be gridded
        (default: the image's)
    :param normalise: divide by the sum of the real parts of the central
        kernel (chan 0, pol 0, w = 0, offset 0)
    :return: (gcf Image, cf ConvolutionFunction)
    """
    g = cf_geometry(im, nw, wstep, oversampling, support, farfield_npixel, pb, polarisation_frame)
    cf_wcs = cf_wcs_for_image(im, g["nw"], wstep, g["os"], g["support"])
    gcf_host = grid_correction_pixels(g["nchan"], g["npol"], g["nx"], use_aaf)

    dev = _device.device()
    ref = im["pixels"].data
    n, nd, sup = g["N"], g["nd"], g["support"]
    taper = None
    if use_aaf:
        taper = _device.to_dev(grdsf(np.abs(2 * coordinates(n)))[0], torch.float64, dev)
    pbd = None
    if pb is not None:
        pbd = _device.to_dev(pb, torch.complex128, dev).reshape(-1, n, n).contiguous()
    w = torch.as_tensor(g["w"], dtype=torch.float64, device=dev)
    cf = kernels.wkernel_create(n, g["os"], sup, w, g["fov"], taper=taper, pb=pbd)
    if normalise:
        cf = cf / torch.sum(cf[0, g["nw"] // 2, g["h"], g["h"]].real)
    tail = (g["nw"], nd, nd, sup, sup)
    if pb is None:
        cf = cf.reshape((1, 1) + tail).expand((g["nchan"], g["npol"]) + tail)
    else:
        cf = cf.reshape((g["nchan"], g["npol"]) + tail)
    if _device.is_device(ref):
        cf_pixels = cf
        gcf_pixels = _device.to_dev(gcf_host, torch.float64, dev)
    else:
        cf_pixels = np.ascontiguousarray(cf.cpu().numpy())
        gcf_pixels = gcf_host
    gcf = Image.constructor(gcf_pixels, g["frame"], im.image_acc.wcs.deepcopy())
    return gcf, ConvolutionFunction.constructor(cf_pixels, cf_wcs, g["frame"])


def create_pswf_convolutionfunction(im, oversampling=8, support=6, polarisation_frame=None):
    """Grid correction and oversampled spheroidal (anti-aliasing only)
    convolution function for ``im``: create_awterm_convolutionfunction with one
    plane at w = 0.  Not in the reference.

    :return: (gcf Image, cf ConvolutionFunction)
    """
    return create_awterm_convolutionfunction(im, nw=1, wstep=1e15, oversampling=oversampling,
                                             support=support, use_aaf=True,
                                             polarisation_frame=polarisation_frame)
