"""Imaging helpers around the hot path (reference src/ska_sdp_func_python/imaging/base.py).

* ``shift_vis_to_image`` (:48-92): rotate to the image centre pixel
  (nx//2+1, ny//2+1, 1-based) when it differs from the vis phase centre.
* ``normalise_sumwt`` (:95-155): divide each [chan, pol] plane by sumwt, or
  zero it when sumwt <= 0 (2-D sumwt); the 4-D (image) form follows :129-149.
* ``predict_awprojection`` / ``invert_awprojection`` (:158-259) over the HIP
  convolution-function gridder (grid_data.gridding).
* ``fill_vis_for_psf`` (:262-296).
* ``create_image_from_visibility`` (:299-438), ``advise_wide_field`` (:441-790),
  ``rad_deg_arcsec`` (:793-802) and ``visibility_recentre`` (:805-815): the
  reference's arithmetic on the host.  Their only reductions, max |uvw| over the
  rows, run with torch where the Visibility's uvw is a device tensor.
"""

import logging

import numpy as np
import torch

from .. import _device
from ..datamodels import (C_M_S, PolarisationFrame, create_griddata_from_image, create_image,
                          pixel_to_skycoord)
from ..util.coordinate_support import skycoord_to_lmn
from ..visibility.base import phaserotate_visibility

log = logging.getLogger("func-python-logger")


def shift_vis_to_image(vis, im, tangent=True, inverse=False):
    ny = im["pixels"].data.shape[2]
    nx = im["pixels"].data.shape[3]
    image_phasecentre = pixel_to_skycoord(nx // 2 + 1, ny // 2 + 1, im.image_acc.wcs, origin=1)
    if vis.phasecentre.separation(image_phasecentre).rad > 1e-15:
        if inverse:
            log.debug("shift_vis_from_image: shifting phasecentre from image phase centre %s "
                      "to visibility phasecentre %s", image_phasecentre, vis.phasecentre)
        else:
            log.debug("shift_vis_from_image: shifting phasecentre from vis phasecentre %s to "
                      "image phasecentre %s", vis.phasecentre, image_phasecentre)
        vis = phaserotate_visibility(vis, image_phasecentre, tangent=tangent, inverse=inverse)
        vis.attrs["phasecentre"] = im.image_acc.phasecentre
    return vis


def shift_lmn(vis, im):
    """(l, m, n-1) by which ``shift_vis_to_image(vis, im, tangent=True)``
    would rotate the visibilities, or None when it would leave them alone
    (same two tests: phase-centre separation > 1e-15 rad, reference
    imaging/base.py:71-75, and |n-1| >= 1e-15, visibility/base.py:78-82).
    The fused NUFFT entry points apply that rotation on the fly."""
    ny = im["pixels"].data.shape[2]
    nx = im["pixels"].data.shape[3]
    image_phasecentre = pixel_to_skycoord(nx // 2 + 1, ny // 2 + 1, im.image_acc.wcs, origin=1)
    if vis.phasecentre.separation(image_phasecentre).rad <= 1e-15:
        return None
    l, m, n = skycoord_to_lmn(image_phasecentre, vis.phasecentre)
    if abs(n) < 1e-15:
        return None
    return l, m, n


def normalise_sumwt(im, sumwt, min_weight=0.1, flat_sky=False):
    pixels = im["pixels"].data
    nchan, npol = pixels.shape[0], pixels.shape[1]
    assert sumwt is not None
    if isinstance(sumwt, np.ndarray):
        assert nchan == sumwt.shape[0]
        assert npol == sumwt.shape[1]
        for chan in range(nchan):
            for pol in range(npol):
                if sumwt[chan, pol] > 0.0:
                    pixels[chan, pol] = pixels[chan, pol] / sumwt[chan, pol]
                else:
                    pixels[chan, pol] = 0.0
    elif tuple(pixels.shape) == tuple(sumwt["pixels"].data.shape):
        sw = sumwt["pixels"].data
        maxwt = float(sw.max())
        minwt = min_weight * maxwt
        cy, cx = sw.shape[2] // 2, sw.shape[3] // 2
        for chan in range(nchan):
            for pol in range(npol):
                if flat_sky:
                    norm = (sw[chan, pol, cy, cx] * sw[chan, pol]) ** 0.5
                    big = norm > minwt
                    pixels[chan, pol][big] /= norm[big]
                    pixels[chan, pol][~big] /= maxwt
                else:
                    pixels[chan, pol] /= maxwt
                    sw[chan, pol] /= maxwt
                    sumwt["pixels"].data = sw ** 0.5
    else:
        raise ValueError("sumwt is not a 2D or 4D array - cannot perform normalisation")
    im["pixels"].data = pixels
    return im


def fill_vis_for_psf(svis):
    pf = svis.visibility_acc.polarisation_frame
    v = svis["vis"].data
    if pf in (PolarisationFrame("linear"), PolarisationFrame("circular")):
        v[..., 0] = 1.0 + 0.0j
        v[..., 1:3] = 0.0 + 0.0j
        v[..., 3] = 1.0 + 0.0j
    elif pf in (PolarisationFrame("linearnp"), PolarisationFrame("circularnp"),
                PolarisationFrame("stokesI")):
        v[...] = 1.0 + 0.0j
    else:
        raise ValueError(f"Cannot calculate PSF for {pf}")
    return svis


def predict_awprojection(vis, model, gcfcf=None):
    from ..grid_data.gridding import degrid_visibility_from_griddata, fft_image_to_griddata
    from ..image_operations import convert_stokes_to_polimage

    if model is None:
        return vis
    assert not np.isnan(float(np.sum(np.asarray(_host(model["pixels"].data))))), \
        "NaNs present in input model"
    if gcfcf is None:
        raise ValueError("predict_awprojection: gcfcf not specified")
    gcf, cf = gcfcf(model)
    griddata = create_griddata_from_image(model, polarisation_frame=vis.visibility_acc.polarisation_frame)
    polmodel = convert_stokes_to_polimage(model, vis.visibility_acc.polarisation_frame)
    griddata = fft_image_to_griddata(polmodel, griddata, gcf)
    vis = degrid_visibility_from_griddata(vis, griddata=griddata, cf=cf)
    return shift_vis_to_image(vis, model, tangent=True, inverse=True)


def invert_awprojection(vis, im, dopsf=False, normalise=True, gcfcf=None):
    from ..grid_data.gridding import fft_griddata_to_image, grid_visibility_to_griddata
    from ..image_operations import convert_polimage_to_stokes

    svis = vis.copy(deep=True)
    if dopsf:
        svis = fill_vis_for_psf(svis)
    svis = shift_vis_to_image(svis, im, tangent=True, inverse=False)
    griddata = create_griddata_from_image(im, polarisation_frame=vis.visibility_acc.polarisation_frame)
    if gcfcf is None:
        raise ValueError("invert_awprojection: gcfcf not specified")
    gcf, cf = gcfcf(im)
    griddata, sumwt = grid_visibility_to_griddata(svis, griddata=griddata, cf=cf)
    result = fft_griddata_to_image(griddata, im, gcf)
    if normalise:
        result = normalise_sumwt(result, sumwt)
    result = convert_polimage_to_stokes(result)
    assert not np.isnan(float(np.sum(np.asarray(_host(result["pixels"].data))))), \
        "NaNs present in output image"
    return result, sumwt


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def _max_abs(a):
    """numpy.max(numpy.abs(a)) as a float64 scalar; a device tensor is reduced where it lies."""
    if isinstance(a, torch.Tensor):
        return np.float64(torch.amax(torch.abs(a)).item())
    return np.max(np.abs(a))


def create_image_from_visibility(vis, **kwargs):
    """Make an empty template Image consistent with a Visibility (reference
    imaging/base.py:299-438).  The visibilities are not transformed.

    :param vis: Visibility
    :param phasecentre: Phase centre of the image (default: that of ``vis``)
    :param imagecentre: Only logged, as in the reference
    :param frequency: Channel frequencies (Hz; default: those of ``vis``); the first is used
    :param channel_bandwidth: Channel width (Hz; default: the first of ``vis``)
    :param nchan: Number of image channels (default: the number of distinct frequencies)
    :param npixel: Number of pixels on each axis (512)
    :param cellsize: Cell size (radians; default: half the critical one, 1 / (2 uvmax))
    :param override_cellsize: Reset a cell size above the critical one to it (True)
    :param polarisation_frame: default stokesI
    :return: Image
    """
    image_centre = kwargs.get("imagecentre", vis.phasecentre)
    phase_centre = kwargs.get("phasecentre", vis.phasecentre)

    vis_frequency = np.asarray(_host(vis["frequency"].data))
    ufrequency = np.unique(vis_frequency)
    frequency = kwargs.get("frequency", vis_frequency)
    vnchan = len(ufrequency)
    inchan = kwargs.get("nchan", vnchan)
    reffrequency = frequency[0]
    channel_bandwidth = kwargs.get("channel_bandwidth",
                                   np.asarray(_host(vis["channel_bandwidth"].data)).flat[0])

    if (inchan == vnchan) and vnchan > 1:
        mode = f"{inchan} channel Image"
    elif ((inchan == 1) and vnchan > 1) or (inchan > 1 and vnchan > 1) \
            or ((inchan == 1) and (vnchan == 1)):
        assert np.abs(channel_bandwidth) > 0.0, "Channel width must be non-zero for mfs mode"
        mode = "single channel Image" if vnchan == 1 else \
            ("single channel MFS Image" if inchan == 1 else "multi-channel MFS Image")
    else:
        raise ValueError(f"create_image_from_visibility: unknown spectral mode "
                         f"inchan = {inchan}, vnchan = {vnchan}")
    log.debug("create_image_from_visibility: Defining %s at %s, starting frequency %s Hz, and "
              "bandwidth %s Hz", mode, image_centre, reffrequency, channel_bandwidth)

    npixel = kwargs.get("npixel", 512)
    # The reference takes max |uvw_lambda[..., 0:2]| over [time, baseline, chan, 2], whose
    # elements are the rounded products uvw * (frequency / c).  A rounded product of positive
    # numbers is monotone in each factor, so the largest of them is the product of the largest
    # |u|, |v| in metres and the largest frequency / c: the same bits without that array.
    uvmax = _max_abs(vis["uvw"].data[..., 0:2]) * np.max(vis_frequency / C_M_S)
    log.debug("create_image_from_visibility: uvmax = %f wavelengths", uvmax)
    criticalcellsize = 1.0 / (uvmax * 2.0)
    log.debug("create_image_from_visibility: Critical cellsize = %f radians, %f degrees",
              criticalcellsize, criticalcellsize * 180.0 / np.pi)

    cellsize = kwargs.get("cellsize", 0.5 * criticalcellsize)
    log.debug("create_image_from_visibility: Cellsize = %g radians, %g degrees", cellsize,
              cellsize * 180.0 / np.pi)

    override_cellsize = kwargs.get("override_cellsize", True)
    if (override_cellsize and cellsize > criticalcellsize) or (cellsize == 0.0):
        log.debug("create_image_from_visibility: Resetting cellsize %g radians to "
                  "criticalcellsize %g radians", cellsize, criticalcellsize)
        cellsize = criticalcellsize

    pol_frame = kwargs.get("polarisation_frame", PolarisationFrame("stokesI"))
    im = create_image(npixel, cellsize, phase_centre, polarisation_frame=pol_frame,
                      frequency=reffrequency, channel_bandwidth=channel_bandwidth, nchan=inchan)
    log.debug("create_image_from_visibility: image shape is %s", str(im["pixels"].data.shape))
    return im


def advise_wide_field(vis, delA=0.02, oversampling_synthesised_beam=3.0, guard_band_image=6.0,
                      facets=1, verbose=True):
    """Advise on parameters for wide field imaging: the sampling requirements
    that follow from the longest baseline, the largest w, the band and the
    station or dish diameter (reference imaging/base.py:441-790, the same
    arithmetic in the same order and the same keys).

    One deviation: ``npixels_min`` is always what the reference computes when
    pyfftw is not installed, the smallest power of 2, 3, 4 or 5 that reaches
    ``npixels``; with pyfftw the reference returns ``pyfftw.next_fast_len``.

    :param vis: Visibility; ``vis.attrs["configuration"].diameter.data`` holds the diameters
    :param delA: Allowed coherence loss (0.02)
    :param oversampling_synthesised_beam: Oversampling of the synthesized beam (3.0)
    :param guard_band_image: Number of primary beam half-widths-to-half-maximum to image (6)
    :param facets: Number of facets on each axis
    :param verbose: Log every quantity
    :return: Dict of advice
    """
    def say(fmt, *args):
        if verbose:
            log.info("advise_wide_field: " + fmt, *args)

    vis_frequency = np.asarray(_host(vis.frequency.data))
    max_wavelength = C_M_S / np.min(vis_frequency)
    say("(max_wavelength) Maximum wavelength %.3f (meters)", max_wavelength)
    min_wavelength = C_M_S / np.max(vis_frequency)
    say("(min_wavelength) Minimum wavelength %.3f (meters)", min_wavelength)

    maximum_baseline = _max_abs(vis["uvw"].data) / min_wavelength  # wavelengths
    maximum_w = _max_abs(vis.visibility_acc.w.data) / min_wavelength  # wavelengths
    say("(maximum_baseline) Maximum baseline %.1f (wavelengths)", maximum_baseline)
    assert maximum_baseline > 0.0, "Error in UVW coordinates: all uvw are zero"
    say("(maximum_w) Maximum w %.1f (wavelengths)", maximum_w)

    diameter = np.min(vis.attrs["configuration"].diameter.data)
    say("(diameter) Station/dish diameter %.1f (meters)", diameter)
    assert diameter > 0.0, "Station/dish diameter must be greater than zero"

    primary_beam_fov = max_wavelength / diameter
    say("(primary_beam_fov) Primary beam %s", rad_deg_arcsec(primary_beam_fov))
    image_fov = primary_beam_fov * guard_band_image
    say("(image_fov) Image field of view %s", rad_deg_arcsec(image_fov))
    facet_fov = primary_beam_fov * guard_band_image / facets
    if facets > 1:
        say("(facet_fov) Facet field of view %s", rad_deg_arcsec(facet_fov))
    synthesized_beam = 1.0 / (maximum_baseline)
    say("(synthesized_beam) Synthesized beam %s", rad_deg_arcsec(synthesized_beam))
    cellsize = synthesized_beam / oversampling_synthesised_beam
    say("(cellsize) Cellsize %s", rad_deg_arcsec(cellsize))

    def pwr2(n):
        ex = np.ceil(np.log(n) / np.log(2.0)).astype("int")
        return np.power(2, ex)

    def pwr23(n):
        best = pwr2(n)
        if best * 3 // 4 >= n:
            best = best * 3 // 4
        return best

    def pwr2345(n):
        number = np.array([2, 3, 4, 5])
        ex = np.ceil(np.log(n) / np.log(number)).astype("int")
        return min(np.power(number[:], ex[:]))

    npixels = int(round(image_fov / cellsize))
    say("(npixels) Npixels per side = %d", npixels)
    npixels2 = pwr2(npixels)
    say("(npixels2) Npixels (power of 2) per side = %d", npixels2)
    npixels23 = pwr23(npixels)
    say("(npixels23) Npixels (power of 2, 3) per side = %d", npixels23)
    npixels_min = pwr2345(npixels)
    say("(npixels_min) Npixels (power of 2, 3, 4, 5) per side = %d", npixels_min)

    # Cornwell, Humphreys and Voronkov (2012), equation 24, with the constraint
    # held at one quarter of the field of view
    w_sampling_image = np.sqrt(2.0 * delA) / (np.pi * image_fov**2)
    say("(w_sampling_image) W sampling for full image = %.1f (wavelengths)", w_sampling_image)
    if facets > 1:
        w_sampling_facet = np.sqrt(2.0 * delA) / (np.pi * facet_fov**2)
        say("(w_sampling_facet) W sampling for facet = %.1f (wavelengths)", w_sampling_facet)
    else:
        w_sampling_facet = w_sampling_image
    w_sampling_primary_beam = np.sqrt(2.0 * delA) / (np.pi * primary_beam_fov**2)
    say("(w_sampling_primary_beam) W sampling for primary beam = %.1f (wavelengths)",
        w_sampling_primary_beam)

    time_sampling_image = 86400.0 * (synthesized_beam / image_fov)
    say("(time_sampling_image) Time sampling for full image = %.1f (s)", time_sampling_image)
    if facets > 1:
        time_sampling_facet = 86400.0 * (synthesized_beam / facet_fov)
        say("(time_sampling_facet) Time sampling for facet = %.1f (s)", time_sampling_facet)
    else:
        time_sampling_facet = time_sampling_image
    time_sampling_primary_beam = 86400.0 * (synthesized_beam / primary_beam_fov)
    say("(time_sampling_primary_beam) Time sampling for primary beam = %.1f (s)",
        time_sampling_primary_beam)

    max_freq = np.max(vis_frequency)
    freq_sampling_image = max_freq * (synthesized_beam / image_fov)
    say("(freq_sampling_image) Frequency sampling for full image = %.1f (Hz)", freq_sampling_image)
    if facets > 1:
        freq_sampling_facet = max_freq * (synthesized_beam / facet_fov)
        say("(freq_sampling_facet) Frequency sampling for facet = %.1f (Hz)", freq_sampling_facet)
    else:
        freq_sampling_facet = freq_sampling_image
    freq_sampling_primary_beam = max_freq * (synthesized_beam / primary_beam_fov)
    say("(freq_sampling_primary_beam) Frequency sampling for primary beam = %.1f (Hz)",
        freq_sampling_primary_beam)

    wstep_primary_beam = w_sampling_primary_beam
    vis_slices_primary_beam = max(1, int(2 * maximum_w / wstep_primary_beam))
    wprojection_planes_primary_beam = vis_slices_primary_beam
    nwpixels_primary_beam = int(2.0 * wprojection_planes_primary_beam * primary_beam_fov)
    nwpixels_primary_beam = nwpixels_primary_beam - nwpixels_primary_beam % 2
    say("(vis_slices_primary_beam) Number of planes in w stack %d (primary beam)",
        vis_slices_primary_beam)
    say("(wprojection_planes_primary_beam) Number of planes in w projection %d (primary beam)",
        wprojection_planes_primary_beam)
    say("(nwpixels_primary_beam) W support = %d (pixels) (primary beam)", nwpixels_primary_beam)

    wstep_image = w_sampling_image
    vis_slices_image = max(1, int(2 * maximum_w / wstep_image))
    wprojection_planes_image = vis_slices_image
    nwpixels_image = int(2.0 * wprojection_planes_image * image_fov)
    nwpixels_image = nwpixels_image - nwpixels_image % 2
    say("(vis_slices_image) Number of planes in w stack %d (image)", vis_slices_image)
    say("(wprojection_planes_image) Number of planes in w projection %d (image)",
        wprojection_planes_image)
    say("(nwpixels_image) W support = %d (pixels) (image)", nwpixels_image)
    say("by default, using primary beam to advise on w sampling parameters")

    return {
        "delA": delA,
        "oversampling_synthesised_beam": oversampling_synthesised_beam,
        "guard_band_image": guard_band_image,
        "facets": facets,
        "verbose": verbose,
        "max_wavelength": max_wavelength,
        "min_wavelength": min_wavelength,
        "maximum_baseline": maximum_baseline,
        "maximum_w": maximum_w,
        "diameter": diameter,
        "primary_beam_fov": primary_beam_fov,
        "image_fov": image_fov,
        "facet_fov": facet_fov,
        "synthesized_beam": synthesized_beam,
        "cellsize": cellsize,
        "npixels": npixels,
        "npixels2": npixels2,
        "npixels23": npixels23,
        "npixels_min": npixels_min,
        "w_sampling_image": w_sampling_image,
        "w_sampling_facet": w_sampling_facet,
        "w_sampling_primary_beam": w_sampling_primary_beam,
        "time_sampling_image": time_sampling_image,
        "time_sampling_primary_beam": time_sampling_primary_beam,
        "max_freq": max_freq,
        "freq_sampling_image": freq_sampling_image,
        "freq_sampling_primary_beam": freq_sampling_primary_beam,
        "wstep_primary_beam": wstep_primary_beam,
        "vis_slices_primary_beam": vis_slices_primary_beam,
        "wprojection_planes_primary_beam": wprojection_planes_primary_beam,
        "nwpixels_primary_beam": nwpixels_primary_beam,
        "wstep_image": wstep_image,
        "vis_slices_image": vis_slices_image,
        "wprojection_planes_image": wprojection_planes_image,
        "nwpixels_image": nwpixels_image,
    }


def rad_deg_arcsec(x):
    """Stringify an angle x (radians) in radians, degrees and arcseconds."""
    return (f"{x:.3g} (rad) {180.0 * x / np.pi:.3g} (deg) "
            f"{3600.0 * 180.0 * x / np.pi:.3g} (asec)")


def visibility_recentre(uvw, dl, dm):
    """Compensate for kernel re-centring, see ``w_kernel_function``
    (reference imaging/base.py:805-815).

    :param uvw: Visibility coordinates [n, 3], numpy or a device tensor
    :param dl: Horizontal shift to compensate for
    :param dm: Vertical shift to compensate for
    :return: Visibility coordinates re-centred on the peak of their w-kernel
    """
    if isinstance(uvw, torch.Tensor):
        u, v, w = torch.hsplit(uvw, 3)
        return torch.hstack([u - w * dl, v - w * dm, w])
    u, v, w = np.hsplit(uvw, 3)
    return np.hstack([u - w * dl, v - w * dm, w])
