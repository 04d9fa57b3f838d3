"""Sky-component operations (reference
src/ska_sdp_func_python/sky_component/operations.py).

apply_beam_to_skycomponent (:366-444) is host logic over a handful of
components: each point component's flux is multiplied (or, with ``inverse``
and a non-zero beam, divided) by the beam pixel its direction projects to
(SIN projection, origin 1, Python's round-half-even); components off the
image get zero flux.

insert_skycomponent (:583-668), restore_skycomponent (:671-741),
voronoi_decomposition (:744-783) and image_voronoi_iter (:786-815) work on
the image: the host computes what is O(components) -- pixel locations, fluxes
per image channel, the interpolation taps -- with the reference's arithmetic,
and the pixels are updated by csrc/skycomp.hip.  An image whose pixels are a
device tensor is updated in place and stays on the device; numpy pixels go
through the device and are updated in place too.

find_skycomponents (:256-363) turns an image back into components: channel
mean, smoothing, 8-connected segmentation and the per-channel peak search run
on the device (csrc/segment.hip), the O(segments x channels) rest on the host.
segment_image returns its segment map.  The catalogue helpers that follow a
find (:65-253, :565-580, :818-832, :919-943) are small host functions;
astropy's catalogue matching is replaced by SkyCoord.separation.

fit_skycomponent (:835-916) fits a rotated Gaussian to the 15 x 15 pixels about
a component: the fit runs on the device (csrc/gaussfit.hip, one wavefront per
window), the O(components) rest -- window placement, direction, the pixel the
flux is read at, shape and params -- on the host in fitted_skycomponent.
fit_skycomponents does the fits of many components in many images in one launch.
"""

import collections.abc
import copy
import logging

import numpy as np
from scipy import interpolate

from .. import _device, kernels
from ..datamodels import Image, SkyComponent, SkyCoord, pixel_to_skycoord, skycoord_to_pixel
from ..image.operations import convert_clean_beam_to_pixels

__all__ = ["apply_beam_to_skycomponent", "insert_skycomponent", "restore_skycomponent",
           "voronoi_decomposition", "image_voronoi_iter", "insert_function_sinc",
           "insert_function_L", "insert_function_pswf", "grdsf", "find_skycomponents",
           "segment_image", "segment_kernel", "find_nearest_skycomponent_index",
           "find_nearest_skycomponent", "find_separation_skycomponents",
           "find_skycomponent_matches_atomic", "find_skycomponent_matches",
           "select_components_by_separation", "remove_neighbouring_components",
           "filter_skycomponents_by_flux", "fit_skycomponent_spectral_index",
           "fit_skycomponent", "fit_skycomponents", "fitted_skycomponent",
           "select_neighbouring_components", "partition_skycomponent_neighbours"]

log = logging.getLogger("func-python-logger")


def apply_beam_to_skycomponent(sc, beam, phasecentre=None, inverse=False):
    single = not isinstance(sc, collections.abc.Iterable)
    if single:
        sc = [sc]
    ny = beam["pixels"].data.shape[2]
    nx = beam["pixels"].data.shape[3]
    pixels = beam["pixels"].data
    pixels = pixels.cpu().numpy() if hasattr(pixels, "cpu") else np.asarray(pixels)
    log.debug("apply_beam_to_skycomponent: Processing %d components", len(sc))
    wcs = beam.image_acc.wcs
    if wcs.wcs.ctype[0] != "RA---SIN":
        wcs = copy.deepcopy(wcs)
        wcs.wcs.ctype[0] = "RA---SIN"
        wcs.wcs.ctype[1] = "DEC--SIN"
        wcs.wcs.crval[0] = phasecentre.ra.deg
        wcs.wcs.crval[1] = phasecentre.dec.deg
    pixlocs = skycoord_to_pixel([c.direction for c in sc], wcs, origin=1, mode="wcs")
    newsc = []
    total_flux = np.zeros_like(sc[0].flux)
    for icomp, comp in enumerate(sc):
        assert comp.shape == "Point", f"Cannot handle shape {comp.shape}"
        pixloc = (pixlocs[0][icomp], pixlocs[1][icomp])
        if not np.isnan(pixloc).any():
            x, y = int(round(float(pixloc[0]))), int(round(float(pixloc[1])))
            if 0 <= x < nx and 0 <= y < ny:
                if inverse and (pixels[:, :, y, x] != 0.0).all():
                    comp_flux = comp.flux / pixels[:, :, y, x]
                else:
                    comp_flux = comp.flux * pixels[:, :, y, x]
                total_flux += comp_flux
            else:
                comp_flux = 0.0 * comp.flux
            newsc.append(SkyComponent(comp.direction, comp.frequency, comp.name, comp_flux,
                                      shape=comp.shape, polarisation_frame=comp.polarisation_frame))
    log.debug("apply_beam_to_skycomponent: %d components with total flux %s", len(newsc),
              total_flux)
    if single:
        return newsc[0]
    return newsc


# ---- insert functions (util/array_functions.py:102-131, fft_coordinates.py grdsf)
# Schwab's rational approximation of the spheroidal function (m = 6, alpha = 1):
# numerator and denominator coefficients in nu^2 - nuend^2 for nu < 0.75 and
# for 0.75 <= nu <= 1
_GRDSF_P = np.array([[8.203343e-2, -3.644705e-1, 6.278660e-1, -5.335581e-1, 2.312756e-1],
                     [4.028559e-3, -3.697768e-2, 1.021332e-1, -1.201436e-1, 6.412774e-2]])
_GRDSF_Q = np.array([[1.0000000e0, 8.212018e-1, 2.078043e-1],
                     [1.0000000e0, 9.599102e-1, 2.918724e-1]])


def grdsf(nu):
    """The spheroidal function at the 1-D array ``nu`` (distance to the edge):
    (the grid-correction function, the gridding function (1 - nu^2) times it);
    0 beyond nu = 1.  The reference's arithmetic, operation by operation."""
    nu = np.abs(nu)
    lower = (nu >= 0.0) & (nu < 0.75)
    upper = (nu >= 0.75) & (nu <= 1.0)
    part = np.zeros(len(nu), dtype="int")
    part[upper] = 1
    nuend = np.zeros_like(nu)
    nuend[lower] = 0.75
    nuend[upper] = 1.0
    delnusq = nu**2 - nuend**2
    top = _GRDSF_P[part, 0]
    for k in range(1, _GRDSF_P.shape[1]):
        top += _GRDSF_P[part, k] * np.power(delnusq, k)
    bot = _GRDSF_Q[part, 0]
    for k in range(1, _GRDSF_Q.shape[1]):
        bot += _GRDSF_Q[part, k] * np.power(delnusq, k)
    value = np.zeros_like(nu)
    ok = bot > 0.0
    value[ok] = top[ok] / bot[ok]
    value[nu > 1.0] = 0.0
    return value, (1 - nu**2) * value


def insert_function_sinc(x):
    """sin(pi x) / (pi x), and -- as in the reference -- 0 at x == 0."""
    s = np.zeros_like(x)
    nz = x != 0.0
    s[nz] = np.sin(np.pi * x[nz]) / (np.pi * x[nz])
    return s


def insert_function_L(x, a=5):
    """Lanczos: sinc(x) sinc(x / a)."""
    return insert_function_sinc(x) * insert_function_sinc(x / a)


def insert_function_pswf(x, a=5):
    """The spheroidal gridding function of |x| / a."""
    return grdsf(abs(x) / a)[1]


_INSERT_FUNCTIONS = {"Lanczos": insert_function_L, "Sinc": insert_function_sinc,
                     "PSWF": insert_function_pswf}


def insert_taps(x, y, bandwidth, support, insert_function):
    """insert_array's host part for one component at pixel (x, y): the window's
    first pixel (x0, y0), the row and column taps (length 2 * support) and the
    sum of their outer product, which the weights are divided by."""
    intx = int(np.round(x))
    inty = int(np.round(y))
    fracx = x - intx
    fracy = y - inty
    grid = np.arange(-support, support)
    taps_y = insert_function(bandwidth * (grid - fracy))
    taps_x = insert_function(bandwidth * (grid - fracx))
    insertsum = np.sum(np.outer(taps_y, taps_x))
    assert insertsum > 0, f"Sum of interpolation coefficients {insertsum}."
    return (intx - support, inty - support), taps_y, taps_x, insertsum


# ---- shared host steps -------------------------------------------------------
def _component_list(sc, who):
    if not isinstance(sc, collections.abc.Iterable):
        sc = [sc]
    sc = list(sc)
    for comp in sc:
        if comp.shape != "Point":
            raise ValueError(f"{who}: Cannot handle shape {comp.shape}")
    return sc


def _image_flux(comp, image_frequency, nchan, npol, as_is_on_equal_frequencies):
    """The component's flux on the image's channels [nchan, npol]: cubic
    interpolation in frequency when it has more than one channel (restore:
    unless its frequencies are the image's within 1e-7), else broadcast."""
    cfreq = np.asarray(comp.frequency, dtype=float)
    flux = np.asarray(comp.flux)
    same = (as_is_on_equal_frequencies and len(cfreq) == len(image_frequency)
            and np.max(np.abs(cfreq - image_frequency)) < 1e-7)
    if not same and flux.shape[0] > 1:
        out = np.zeros([nchan, npol])
        for pol in range(npol):
            out[:, pol] = interpolate.interp1d(cfreq, flux[:, pol], kind="cubic")(image_frequency)
        return out
    flux = np.asarray(flux, dtype=np.float64)
    return flux if flux.shape == (nchan, npol) else np.broadcast_to(flux, (nchan, npol))


def _check_pixels(pixels, who):
    if len(pixels.shape) != 4 or str(pixels.dtype).split(".")[-1] not in ("float32", "float64"):
        raise ValueError(f"{who}: the image must be float32 or float64 [nchan, npol, ny, nx]")
    return tuple(int(n) for n in pixels.shape)


def _update_pixels(pixels, op):
    """Run ``op`` (in place on a contiguous device tensor) on the image's pixels
    where they are: a device tensor is updated in its own storage, host pixels
    travel to the device and back into the same array."""
    import torch
    if _device.is_device(pixels):
        t = pixels if pixels.is_contiguous() else pixels.contiguous()
        op(t)
        if t is not pixels:
            pixels.copy_(t)
        return
    t = _device.to_dev(pixels)
    op(t)
    if isinstance(pixels, torch.Tensor):
        pixels.copy_(t.cpu())
    else:
        pixels[...] = t.cpu().numpy()


# ---- insert_skycomponent -----------------------------------------------------
def insert_skycomponent(im, sc, insert_method="Nearest", bandwidth=1.0, support=8):
    """Insert point SkyComponents into an Image, in place (reference :583-668).

    "Nearest" adds each component's flux to the pixel nearest to it
    (numpy.round, half to even); "Sinc", "Lanczos" and "PSWF" spread it over a
    window of ``2 * int(support / bandwidth)`` pixels a side with the reference's
    interpolation functions, normalised to unit sum; any other name acts as
    "Nearest", as in the reference.  The flux on the image's channels is the
    component's, cubic-interpolated in frequency when it has more than one
    channel.  All components are added by one gather kernel in which every
    pixel adds its terms in component order, so the image is the reference's
    sequential result bit for bit.

    Where this differs from the reference:

    * a "Sinc" / "Lanczos" / "PSWF" component whose window does not lie wholly
      on the image (or which has no pixel location) raises ``ValueError`` before
      any pixel is changed; the reference fails with numpy's broadcast
      ``ValueError`` after inserting the earlier components, and for a window
      wholly left of or above the image wraps round silently;
    * a single-channel component flux is broadcast over the image's channels
      for every method (the reference: only for "Nearest", ``IndexError``
      otherwise);
    * "Nearest" components off the image, or without a pixel location (behind
      the tangent plane), are skipped, counted and logged as in the reference;
    * a shape other than "Point" raises ``ValueError`` before any pixel is
      changed.

    :param im: Image; pixels float64 or float32, numpy or a device tensor
    :param sc: SkyComponent or list of SkyComponents
    :param insert_method: "Nearest" | "Sinc" | "Lanczos" | "PSWF"
    :param bandwidth: fraction of the uv plane to optimise over
    :param support: support of the interpolation function
    :return: the same Image
    """
    support = int(support / bandwidth)
    pixels = im["pixels"].data
    nchan, npol, ny, nx = _check_pixels(pixels, "insert_skycomponent")
    sc = _component_list(sc, "insert_skycomponent")
    log.debug("insert_skycomponent: Using insert method %s", insert_method)
    if not sc:
        return im
    image_frequency = np.asarray(im.frequency.data)
    px, py = skycoord_to_pixel([comp.direction for comp in sc], im.image_acc.wcs, origin=0,
                               mode="wcs")
    flux = np.stack([_image_flux(comp, image_frequency, nchan, npol, False) for comp in sc])
    insert_function = _INSERT_FUNCTIONS.get(insert_method)
    nbad = 0
    if insert_function is None:
        with np.errstate(invalid="ignore"):
            x, y = np.round(px), np.round(py)
            on = np.isfinite(x) & np.isfinite(y) & (x >= 0) & (x < nx) & (y >= 0) & (y < ny)
        nbad = int(len(sc) - np.count_nonzero(on))
        origin = np.stack([x[on], y[on]], axis=1).astype("int")
        taps_y = taps_x = np.ones([len(origin), 1])
        insertsum = np.ones(len(origin))
        flux = flux[on]
    else:
        origin, taps_y, taps_x, insertsum = [], [], [], []
        for icomp in range(len(sc)):
            if not (np.isfinite(px[icomp]) and np.isfinite(py[icomp])):
                raise ValueError(f"insert_skycomponent: component {icomp} has no pixel location")
            o, ty, tx, s = insert_taps(px[icomp], py[icomp], bandwidth, support, insert_function)
            if o[0] < 0 or o[1] < 0 or o[0] + 2 * support > nx or o[1] + 2 * support > ny:
                raise ValueError(
                    f"insert_skycomponent: the {2 * support}-pixel window of component {icomp} "
                    f"at pixel ({px[icomp]:.2f}, {py[icomp]:.2f}) does not fit on the image")
            origin.append(o)
            taps_y.append(ty)
            taps_x.append(tx)
            insertsum.append(s)
        origin, taps_y, taps_x = np.array(origin), np.array(taps_y), np.array(taps_x)
        insertsum = np.array(insertsum)
    if len(origin):
        _update_pixels(pixels, lambda t: kernels.skycomp_insert(t, origin, taps_y, taps_x,
                                                                insertsum, flux))
    if nbad > 0:
        log.warning("insert_skycomponent: %s components of %s do not fit on image", nbad, len(sc))
    return im


# ---- restore_skycomponent ----------------------------------------------------
def restore_skycomponent(im, sc, clean_beam=None):
    """Add point SkyComponents to an Image as clean-beam Gaussians of their
    flux, in place (reference :671-741).

    Each component adds flux * exp(-(a dx^2 + b dx dy + c dy^2)) about its
    (fractional) pixel, with a, b, c of the clean beam in pixels (astropy's
    Gaussian2D).  The flux is the component's as is when its frequencies are
    the image's within 1e-7, else cubic-interpolated when it has more than
    one channel, else broadcast.  One kernel adds all components, per pixel
    in component order; a component is skipped on an image tile only where
    the exponent's argument exceeds 700 (a factor below 1e-304) on all of it,
    so a component off the image still adds its tail.  A component without a
    pixel location (behind the tangent plane) raises ``ValueError``; the
    reference fills the image with NaN.

    :param im: Image; pixels float64 or float32, numpy or a device tensor
    :param sc: SkyComponent or list of SkyComponents
    :param clean_beam: {"bmaj", "bmin", "bpa"} in (deg, deg, deg)
    :return: the same Image, ``attrs["clean_beam"]`` set
    """
    from ..image.deconvolution import _gaussian_coefficients
    pixels = im["pixels"].data
    nchan, npol, ny, nx = _check_pixels(pixels, "restore_skycomponent")
    sc = _component_list(sc, "restore_skycomponent")
    if clean_beam is None:
        raise ValueError("restore_skycomponent: the clean_beam must be specified")
    beam_pixels = convert_clean_beam_to_pixels(im, clean_beam)
    a, b, c = _gaussian_coefficients(float(beam_pixels[0]), float(beam_pixels[1]),
                                     float(beam_pixels[2]))
    if sc:
        image_frequency = np.asarray(im.frequency.data)
        px, py = skycoord_to_pixel([comp.direction for comp in sc], im.image_acc.wcs, origin=0,
                                   mode="wcs")
        if not (np.isfinite(px).all() and np.isfinite(py).all()):
            raise ValueError("restore_skycomponent: a component has no pixel location")
        flux = np.stack([_image_flux(comp, image_frequency, nchan, npol, True) for comp in sc])
        xy = np.stack([px, py], axis=1)
        _update_pixels(pixels, lambda t: kernels.skycomp_restore(t, xy, flux, a, b, c))
    im.attrs["clean_beam"] = clean_beam
    return im


# ---- Voronoi -----------------------------------------------------------------
def voronoi_decomposition(im, comps):
    """The Voronoi decomposition of an image by a set of components (reference
    :744-783): scipy's Voronoi structure of the components' pixel positions
    (host) and the label image [ny, nx] of each pixel's nearest component,
    argmin of hypot with the first minimum on ties -- integers, on the
    image's device when its pixels are a device tensor, else numpy.  As in
    the reference, the positions are 1-based pixels and are compared with
    0-based pixel indices.

    :param im: Image
    :param comps: list of SkyComponents
    :return: Voronoi structure, label image
    """
    from scipy.spatial import Voronoi
    x, y = skycoord_to_pixel([c.direction for c in comps], im.image_acc.wcs, 1, "wcs")
    points = [(x_elem, y[i]) for i, x_elem in enumerate(x)]
    vor = Voronoi(points)
    pixels = im["pixels"].data
    ny, nx = int(pixels.shape[2]), int(pixels.shape[3])
    dev = pixels.device if _device.is_device(pixels) else _device.device()
    labels = kernels.skycomp_nearest(ny, nx, vor.points, dev)
    return vor, _device.like_input(labels, pixels)


def image_voronoi_iter(im, components):
    """Generator of the Voronoi regions of ``components`` as full-size mask
    Images (1.0 inside, 0.0 outside, float64; reference :786-815): region
    0 .. max label; one all-ones mask for a single component.  The masks of a
    device image are built on its device."""
    import torch
    pixels = im["pixels"].data
    on_device = _device.is_device(pixels)
    shape = tuple(int(n) for n in pixels.shape)

    def image_of(mask):
        return Image.constructor(data=mask, polarisation_frame=im.image_acc.polarisation_frame,
                                 wcs=im.image_acc.wcs)

    if len(components) == 1:
        yield image_of(torch.ones(shape, dtype=torch.float64, device=pixels.device) if on_device
                       else np.ones(shape))
        return
    _, labels = voronoi_decomposition(im, components)
    nregions = int(labels.max()) + 1
    for region in range(nregions):
        if on_device:
            mask = (labels == region).to(torch.float64).expand(shape).contiguous()
        else:
            mask = np.zeros(shape)
            mask[:, :, (labels == region)] = 1.0
        yield image_of(mask)


# ---- find_skycomponents ----------------------------------------------------------
def segment_kernel(fwhm):
    """The smoothing kernel of find_skycomponents (:278-284): a Gaussian of the
    given FWHM in pixels sampled at integer offsets on ``int(1.5 * fwhm)``
    pixels a side, one more when that is even, normalised to unit sum."""
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    size = int(1.5 * fwhm)
    if size % 2 == 0:
        size += 1
    if size > kernels.SEGMENT_KERNEL_MAX:
        raise ValueError(f"find_skycomponents: fwhm {fwhm} asks for a smoothing kernel of {size} "
                         f"pixels a side; at most {kernels.SEGMENT_KERNEL_MAX} are supported")
    if size == 1:
        return np.ones((1, 1))
    offsets = np.arange(size) - size // 2
    r2 = offsets[:, None] ** 2 + offsets[None, :] ** 2
    g = np.exp(-r2 / (2.0 * sigma ** 2))
    return g / g.sum()


def _segments(im, fwhm, threshold, npixels, who):
    """The image's pixels on the device, their Stokes-I planes [nchan, ny, nx],
    the segment map and the number of segments."""
    pixels = im["pixels"].data
    _check_pixels(pixels, who)
    kernel = segment_kernel(fwhm)
    dev_pixels = pixels if _device.is_device(pixels) else _device.to_dev(pixels)
    planes = dev_pixels[:, 0]
    labels, nlabels = kernels.segment_image(planes, threshold, npixels, kernel)
    return dev_pixels, planes, labels, nlabels


def segment_image(im, fwhm=1.0, threshold=1.0, npixels=5):
    """The segment map that find_skycomponents works from: int32 [ny, nx], the
    pixels of segment k (component "Segment k - 1") marked k, the background 0;
    on the image's device when its pixels are a device tensor, else numpy.  An
    image without a segment gives a map of zeros.  Not in the reference.

    :return: segment map, number of segments
    """
    pixels = im["pixels"].data
    _, _, labels, nlabels = _segments(im, fwhm, threshold, npixels, "segment_image")
    return _device.like_input(labels, pixels), nlabels


def find_skycomponents(im, fwhm=1.0, threshold=1.0, npixels=5):
    """Find the components of an Image above a threshold (reference :256-363).

    The mean over the channels of Stokes I is smoothed by a Gaussian of FWHM
    ``fwhm`` pixels and cut into the 8-connected segments of at least
    ``npixels`` pixels above ``threshold`` (photutils' detect_sources).  Each
    segment, in the order of its first pixel, becomes a point SkyComponent
    "Segment k": per channel the brightest Stokes-I pixel of the unsmoothed
    image is found (the first in raster order on ties); direction and pixel
    position are the means over the channels weighted with the absolute peak
    values, and the flux is that of the pixel nearest to the mean position
    (numpy.round), for all channels and polarisations.

    Mean, smoothing, labelling and peak search run on the device
    (csrc/segment.hip); device pixels stay there, and only the per-channel
    peaks and the components' fluxes come to the host.  Where this differs
    from the reference: the pixels must be float32 or float64; a pixel that
    is not finite raises ``ValueError`` (photutils masks it); a smoothing
    kernel of more than 15 pixels a side (fwhm >= 10.67) raises ``ValueError``.
    A segment whose peaks are 0 in every channel has, as in the reference, a
    NaN direction; its flux is then taken at the first channel's peak.

    :param im: Image; pixels float64 or float32, numpy or a device tensor
    :param fwhm: full width at half maximum of the smoothing Gaussian, pixels
    :param threshold: detection threshold on the smoothed mean image
    :param npixels: number of connected pixels a segment needs
    :return: list of SkyComponents, flux a numpy array [nchan, npol]
    """
    import torch
    log.debug("find_skycomponents: Finding components in Image by segmentation")
    dev_pixels, planes, labels, nlabels = _segments(im, fwhm, threshold, npixels,
                                                    "find_skycomponents")
    if nlabels == 0:
        raise ValueError("find_skycomponents: Failed to find any components")
    log.info("find_skycomponents: Identified %d segments", nlabels)
    nx = int(dev_pixels.shape[3])
    values, indices = kernels.segment_peaks(planes, labels, nlabels)
    values, indices = values.cpu().numpy(), indices.cpu().numpy()
    wcs = im.image_acc.wcs
    directions, cols, rows = [], [], []
    all_xs, all_ys = (indices % nx).astype(float), (indices // nx).astype(float)
    world = {}  # peak pixel -> (ra, dec): the channels of a segment mostly share theirs
    for segment in range(nlabels):
        flux = values[:, segment]
        xs, ys = all_xs[:, segment], all_ys[:, segment]
        for pixel, x, y in zip(indices[:, segment].tolist(), xs, ys):
            if pixel not in world:
                c = pixel_to_skycoord(x, y, wcs, 0)
                world[pixel] = (c.ra.rad, c.dec.rad)
        ras = np.array([world[pixel][0] for pixel in indices[:, segment].tolist()])
        decs = np.array([world[pixel][1] for pixel in indices[:, segment].tolist()])
        aflux = np.abs(flux)
        flux_sum = np.sum(aflux)
        with np.errstate(invalid="ignore", divide="ignore"):
            ra = np.sum(aflux * ras) / flux_sum
            dec = np.sum(aflux * decs) / flux_sum
            x = np.sum(aflux * xs) / flux_sum
            y = np.sum(aflux * ys) / flux_sum
        if not (np.isfinite(x) and np.isfinite(y)):
            x, y = xs[0], ys[0]
        directions.append(SkyCoord(ra, dec))
        cols.append(int(np.round(x)))
        rows.append(int(np.round(y)))
    at = lambda v: torch.as_tensor(v, dtype=torch.int64, device=dev_pixels.device)
    point_flux = dev_pixels[:, :, at(rows), at(cols)].permute(2, 0, 1).cpu().numpy()
    frequency = np.asarray(im.frequency.data)
    return [SkyComponent(direction=directions[k], frequency=frequency, name=f"Segment {k}",
                         flux=point_flux[k], shape="Point",
                         polarisation_frame=im.image_acc.polarisation_frame, params={})
            for k in range(nlabels)]


# ---- fit_skycomponent ---------------------------------------------------------------
FIT_HALF_WINDOW = kernels.GAUSS_FIT_WINDOW // 2
_SIGMA_TO_FWHM = 2.0 * np.sqrt(2.0 * np.log(2.0))


def _image_x(im):
    """The image's "x" coordinate as ska-sdp-datamodels' Image builds it, in
    degrees: nx points from crval - cdelt nx / 2 in steps of cdelt."""
    w = im.image_acc.wcs.wcs
    nx = int(im["pixels"].data.shape[3])
    cellsize = np.abs(w.cdelt[1])
    return np.linspace(w.crval[0] - cellsize * nx / 2, w.crval[0] + cellsize * nx / 2, nx,
                       endpoint=False)


def fitted_skycomponent(im, sc, params, status, flux_at, **kwargs):
    """The host half of fit_skycomponent (reference :854-916): the component
    that the fit's parameters make of ``sc``.

    :param im: Image (its WCS and shape are used, not its pixels)
    :param sc: the SkyComponent that was fitted
    :param params: the fit's (amplitude, x_mean, y_mean, x_stddev, y_stddev,
        theta), the means in 0-based pixels
    :param status: kernels.gauss_fit's status, or None when the window did not
        lie wholly on the image
    :param flux_at: callable (iy, ix) -> the image's pixels[:, :, iy, ix] as a
        numpy array [nchan, npol]; called only for a pixel on the image
    :param force_point_sources: keep the shape "Point" (default True)
    :return: the new SkyComponent; ``sc`` itself when there was no fit
    """
    if status is None:
        log.warning("fit_skycomponent: fit failed  the fitting window of %s does not lie on "
                    "the image", sc.name)
        return sc
    if status == 2:
        log.warning("fit_skycomponent: fit failed  %s: a pixel of the window or an iterate is "
                    "not finite", sc.name)
        return sc
    if status == 1:
        log.warning("fit_skycomponent: the fit of %s reached its iteration limit; the last "
                    "iterate is used", sc.name)
    ny, nx = (int(n) for n in im["pixels"].data.shape[2:])
    x_mean, y_mean = float(params[1]), float(params[2])
    newsc = sc.copy()
    newsc.direction = pixel_to_skycoord(x_mean, y_mean, im.image_acc.wcs, 0)
    iy = round(y_mean)
    ix = round(x_mean)
    # (the reference: "We could fit each frequency separately. For the moment, we just scale")
    if 0 <= iy < ny and 0 <= ix < nx:
        newsc.flux = np.asarray(flux_at(iy, ix))
    try:
        force_point_sources = kwargs["force_point_sources"]
    except KeyError:
        log.info("fit_skycomponent: force_point_sources not give, setting as default: True")
        force_point_sources = True
    x_fwhm = float(params[3]) * _SIGMA_TO_FWHM
    y_fwhm = float(params[4]) * _SIGMA_TO_FWHM
    theta = float(params[5])
    if force_point_sources or (x_fwhm <= 0.0 or y_fwhm <= 0.0):
        newsc.shape = "Point"
    else:
        x = _image_x(im)
        # the reference's cellsize: the span of the x coordinate over its length, not cdelt
        cellsize = np.abs(x[0] - x[-1]) / len(x)
        if y_fwhm > x_fwhm:
            clean_gaussian = {"bmaj": np.rad2deg(y_fwhm * cellsize),
                              "bmin": np.rad2deg(x_fwhm * cellsize),
                              "bpa": np.rad2deg(theta)}
        else:
            clean_gaussian = {"bmaj": np.rad2deg(x_fwhm * cellsize),
                              "bmin": np.rad2deg(y_fwhm * cellsize),
                              "bpa": np.rad2deg(theta) + 90.0}
        newsc.shape = "Gaussian"
        newsc.params = clean_gaussian
    return newsc


def fit_skycomponents(images, comps, **kwargs):
    """Fit every component of ``comps`` in every image of ``images`` with a
    two-dimensional Gaussian: ``len(images) x len(comps)`` fits in one kernel
    launch and one gather of fluxes per image.  Not in the reference, whose
    fit_skycomponent is the 1 x 1 case.

    :param images: an Image or a list of Images; pixels float64 or float32
        [nchan, npol, ny, nx], numpy or device tensors
    :param comps: list of SkyComponents
    :param force_point_sources: keep the shape "Point" (default True)
    :param max_iter: cap on the model evaluations of a fit (default 100)
    :return: list over the images of lists over the components of
        SkyComponents, as fit_skycomponent returns them
    """
    import torch
    images = [images] if isinstance(images, Image) else list(images)
    comps = list(comps)
    max_iter = kwargs.pop("max_iter", 100)
    window = kernels.GAUSS_FIT_WINDOW
    dev_pixels, jobs = [], []   # jobs: (image, component, x0, y0)
    for i, im in enumerate(images):
        pixels = im["pixels"].data
        _, _, ny, nx = _check_pixels(pixels, "fit_skycomponent")
        dev_pixels.append(pixels if _device.is_device(pixels) else _device.to_dev(pixels))
        if not comps:
            continue
        px, py = skycoord_to_pixel([c.direction for c in comps], im.image_acc.wcs, origin=0)
        for k in range(len(comps)):
            if not (np.isfinite(px[k]) and np.isfinite(py[k])):
                continue
            x0 = int(np.round(px[k])) - FIT_HALF_WINDOW
            y0 = int(np.round(py[k])) - FIT_HALF_WINDOW
            if 0 <= x0 and x0 + window <= nx and 0 <= y0 and y0 + window <= ny:
                jobs.append((i, k, x0, y0))
    fits = {}
    for dtype in sorted({t.dtype for t in dev_pixels}, key=str):   # one call per pixel type
        mine = [j for j in jobs if dev_pixels[j[0]].dtype == dtype]
        if not mine:
            continue
        plane = [t[0, 0] for t in dev_pixels]   # one view per image, shared by its fits
        params, status, _ = kernels.gauss_fit([plane[j[0]] for j in mine], [j[2] for j in mine],
                                              [j[3] for j in mine], max_iter)
        params, status = params.cpu().numpy(), status.cpu().numpy()
        for n, (i, k, _, _) in enumerate(mine):
            fits[(i, k)] = (params[n], int(status[n]))
    out = []
    for i, im in enumerate(images):
        ny, nx = (int(n) for n in dev_pixels[i].shape[2:])
        # the pixels that the fitted centres round to, gathered on the device in one go
        wanted = {}
        for k in range(len(comps)):
            if (i, k) in fits and fits[(i, k)][1] != 2:
                iy, ix = round(float(fits[(i, k)][0][2])), round(float(fits[(i, k)][0][1]))
                if 0 <= iy < ny and 0 <= ix < nx:
                    wanted[(iy, ix)] = None
        if wanted:
            at = lambda v: torch.as_tensor(v, dtype=torch.int64, device=dev_pixels[i].device)
            flux = dev_pixels[i][:, :, at([p[0] for p in wanted]), at([p[1] for p in wanted])]
            flux = flux.permute(2, 0, 1).cpu().numpy()
            for n, pixel in enumerate(wanted):
                wanted[pixel] = flux[n]
        row = []
        for k, sc in enumerate(comps):
            params, status = fits.get((i, k), (None, None))
            row.append(fitted_skycomponent(im, sc, params, status,
                                           lambda iy, ix: wanted[(iy, ix)], **kwargs))
        out.append(row)
    return out


def fit_skycomponent(im, sc, **kwargs):
    """Fit a two-dimensional Gaussian to a SkyComponent (reference :835-916).

    Plane [0, 0] of the image is fitted on the 15 x 15 pixels about the pixel
    nearest to the component (numpy.round of its 0-based pixel location) with
    astropy's Gaussian2D, from the reference's start (the window's maximum, its
    centre, standard deviations 1, theta 0), by csrc/gaussfit.hip.  The new
    component has the direction of the fitted centre and the flux of the pixel
    nearest to it (Python's round), all channels and polarisations, when that
    pixel is on the image; its shape is "Point" with ``force_point_sources``
    (default True) or a non-positive width, else "Gaussian" with ``params``
    bmaj, bmin, bpa in degrees as the reference forms them.  Device pixels
    stay on the device: only the six parameters and [nchan, npol] fluxes come
    to the host.

    Where the window does not lie wholly on the image the component is
    returned unchanged and a warning logged, as the reference does through its
    ``except ValueError``.  Where this differs from the reference: a window
    with a pixel that is not finite, or a fit whose iterates leave the finite
    numbers, also returns the component unchanged; the fit is run to a tighter
    stop (a relative step of 1e-12, or a cost that no longer decreases; the
    reference: 1e-7 and 1.49e-8); at the cap of 100 model evaluations the last
    iterate is used and a warning logged; numpy pixels go through the device.

    :param im: Image; pixels float64 or float32, numpy or a device tensor
    :param sc: SkyComponent
    :param force_point_sources: keep the shape "Point" (default True)
    :return: the fitted SkyComponent
    """
    return fit_skycomponents(im, [sc], **kwargs)[0][0]


# ---- catalogue helpers (:65-253, :565-580, :818-832, :919-943) --------------------
# astropy's catalogue matching is replaced by the separations themselves:
# nearest is the smallest separation, the first on ties.
def find_nearest_skycomponent_index(home, comps):
    """The index in ``comps`` of the component nearest to the direction ``home``."""
    if len(comps) == 0:
        raise ValueError("find_nearest_skycomponent_index: Catalog is empty")
    return int(np.argmin([c.direction.separation(home).rad for c in comps]))


def find_nearest_skycomponent(home, comps):
    """The component nearest to ``home`` and its separation in rad."""
    best = comps[find_nearest_skycomponent_index(home, comps)]
    return best, best.direction.separation(home).rad


def find_separation_skycomponents(comps_test, comps_ref=None):
    """The matrix of separations (rad) [ref, test] of two lists of components;
    of ``comps_test`` with itself when ``comps_ref`` is None."""
    if comps_ref is None:
        ncomps = len(comps_test)
        distances = np.zeros([ncomps, ncomps])
        for i in range(ncomps):
            for j in range(i + 1, ncomps):
                distances[i, j] = comps_test[i].direction.separation(comps_test[j].direction).rad
                distances[j, i] = distances[i, j]
        return distances
    separations = np.zeros([len(comps_ref), len(comps_test)])
    for ref, comp_ref in enumerate(comps_ref):
        for test, comp_test in enumerate(comps_test):
            separations[ref, test] = comp_test.direction.separation(comp_ref.direction).rad
    return separations


def find_skycomponent_matches_atomic(comps_test, comps_ref, tol=1e-7):
    """Match candidates to reference components, many to one allowed: the list
    of (test index, nearest reference index, separation) with separation < tol."""
    if len(comps_test) and len(comps_ref) == 0:
        raise ValueError("find_skycomponent_matches: Catalog is empty")
    separations = find_separation_skycomponents(comps_test, comps_ref)
    matches = []
    for test in range(len(comps_test)):
        best = int(np.argmin(separations[:, test]))
        best_sep = separations[best, test]
        if best_sep < tol:
            matches.append((test, best, best_sep))
    return matches


def find_skycomponent_matches(comps_test, comps_ref, tol=1e-7):
    """As find_skycomponent_matches_atomic (the reference's faster variant by
    astropy's catalogue matching; here they are one)."""
    return find_skycomponent_matches_atomic(comps_test, comps_ref, tol)


def select_components_by_separation(home, comps, rmax=2 * np.pi, rmin=0.0):
    """The components whose separation from ``home`` lies in [rmin, rmax] rad."""
    return [comp for comp in comps if rmin <= comp.direction.separation(home).rad <= rmax]


def select_neighbouring_components(comps, target_comps):
    """Assign every component to the nearest target (reference :205-225).

    :return: the index in ``target_comps`` of the target nearest to each
        component (int array) and the separations in rad (float array; the
        reference returns astropy Angles)
    """
    if len(comps) and len(target_comps) == 0:
        raise ValueError("select_neighbouring_components: Catalog is empty")
    separations = find_separation_skycomponents(comps, target_comps)   # [target, comp]
    idx = np.array([int(np.argmin(separations[:, k])) for k in range(len(comps))], dtype=int)
    d2d = np.array([separations[idx[k], k] for k in range(len(comps))], dtype=float)
    return idx, d2d


def partition_skycomponent_neighbours(comps, targets):
    """The components partitioned by their nearest target (reference :818-832):
    one list per target that is nearest to some component, in target order."""
    idx, _ = select_neighbouring_components(comps, targets)
    return [[comp for comp, i in zip(comps, idx) if i == comp_id] for comp_id in np.unique(idx)]


def remove_neighbouring_components(comps, distance):
    """Of two components closer than ``distance`` rad, drop the fainter (by its
    largest flux), pairs taken in list order as in the reference (:228-253).

    :return: indices of the components kept, the components kept
    """
    ncomps = len(comps)
    ok = ncomps * [True]
    for i in range(ncomps):
        if ok[i]:
            for j in range(i + 1, ncomps):
                if ok[j]:
                    d = comps[i].direction.separation(comps[j].direction).rad
                    if d < distance:
                        if np.max(comps[i].flux) > np.max(comps[j].flux):
                            ok[j] = False
                        else:
                            ok[i] = False
                        break
    idx = [i for i in range(ncomps) if ok[i]]
    return idx, [comps[i] for i in idx]


def filter_skycomponents_by_flux(sc, flux_min=-np.inf, flux_max=np.inf):
    """The components whose largest Stokes-I flux lies strictly between the limits."""
    return [comp for comp in sc if flux_min < np.max(comp.flux[:, 0]) < flux_max]


def fit_skycomponent_spectral_index(sc):
    """The spectral index of a multi-frequency component: the slope of log10
    flux (Stokes I) against log10 frequency, both relative to the centre
    channel; 0.0 for a single channel or a centre that is not positive."""
    frequency = np.asarray(sc.frequency, dtype=float)
    nchan = frequency.shape[0]
    if nchan <= 1:
        log.warning("Single frequency skycomponent, skip fitting")
        return 0.0
    centre = nchan // 2
    if frequency[centre] > 0.0 and sc.flux[centre, 0] > 0.0:
        xdata = np.log10(frequency / frequency[centre])
        ydata = np.log10(sc.flux[:, 0] / sc.flux[centre, 0])
        return np.polyfit(xdata, ydata, 1)[0]
    log.warning("Wrong values encountered, no fitting performed.")
    return 0.0
