"""Host restatement of fit_skycomponent (reference
src/ska_sdp_func_python/sky_component/operations.py:835-916) from numpy and
scipy.optimize.leastsq, the stand-in that puts it in place of the kernel
wrapper (kernels.gauss_fit), and the builders of the test cases.  Used by
tests/test_gaussfit_cpu.py, tests/test_gpu_gaussfit.py and
tests/golden/make_golden_gaussfit.py.

This is the yardstick of those tests, and it is NOT a run of the reference:
astropy is not available where this project is built.  It restates, step by
step:

1. the window (:842-849): pixloc = numpy.round(skycoord_to_pixel(direction,
   wcs, origin=0)), rows and columns [pixloc - 7, pixloc + 8) of plane [0, 0];
   where the slices come out short or empty the reference's fit raises
   ValueError and the component is returned unchanged (:912-914);
2. the start (:857-859): astropy 5.2 Gaussian2D(amplitude=max(z),
   x_mean=mean(x), y_mean=mean(y)) with its defaults x_stddev = y_stddev = 1,
   theta = 0;
3. the model: Gaussian2D.evaluate and Gaussian2D.fit_deriv of astropy 5.2
   (modeling/functional_models.py), operation by operation;
4. the bounds: Gaussian2D bounds both standard deviations below by FLOAT_EPSILON
   = float(numpy.finfo(numpy.float32).tiny); astropy 5.2's
   fitter_to_model_params clips the parameters with numpy.fmax before every
   model evaluation and once more on the result, while fit_deriv is called
   with the solver's own (unclipped) vector (fitting._wrap_deriv);
5. the solver: LevMarLSQFitter.__call__ of astropy 5.2 with its defaults
   (maxiter=100, acc=1e-7, epsilon=sqrt(finfo(float).eps)) is
       scipy.optimize.leastsq(objective, p0, Dfun=deriv, col_deriv=True,
                              maxfev=100, xtol=1e-7, epsfcn=epsilon)
   with leastsq's own ftol = 1.49012e-8, the residual model - z unweighted.
   leastsq is MINPACK lmder, the solver the reference runs;
6. the component (:866-910): direction, Python-round pixel, flux, shape and
   params; x_fwhm = x_stddev * 2 sqrt(2 ln 2) (Gaussian2D.x_fwhm).  The image's
   "x" coordinate, which the reference's cellsize is formed from, is
   ska-sdp-datamodels' numpy.linspace(crval - cdelt nx / 2, crval + cdelt nx /
   2, nx, endpoint=False) in degrees.

``tight=True`` runs the same solver to xtol = ftol = 1e-14 with maxfev=2000:
the converged answer that the device fit is compared with.  The largest
difference S between the default and the tight answers over the committed
cases is the scale of the tests' tolerance (2 S).
"""

import contextlib
import os

import numpy as np
from scipy.optimize import leastsq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WINDOW = 15           # SDP_HIP_GAUSS_FIT_WINDOW
HALF = WINDOW // 2
FLOAT_EPSILON = float(np.finfo(np.float32).tiny)
SIGMA_TO_FWHM = 2.0 * np.sqrt(2.0 * np.log(2.0))
NAMES = ("amplitude", "x_mean", "y_mean", "x_stddev", "y_stddev", "theta")
THETA_AXIAL_RATIO = 1.3   # theta is compared for sources at least this elongated
HALF_PIXEL_MARGIN = 0.05  # of a tight centre from a half-integer, in both axes


def load(tag):
    with np.load(os.path.join(GOLDEN, f"gaussfit_{tag}.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


# ---- astropy 5.2 Gaussian2D ------------------------------------------------------
def evaluate(x, y, amplitude, x_mean, y_mean, x_stddev, y_stddev, theta):
    cost2 = np.cos(theta) ** 2
    sint2 = np.sin(theta) ** 2
    sin2t = np.sin(2.0 * theta)
    xstd2 = x_stddev ** 2
    ystd2 = y_stddev ** 2
    xdiff = x - x_mean
    ydiff = y - y_mean
    a = 0.5 * ((cost2 / xstd2) + (sint2 / ystd2))
    b = 0.5 * ((sin2t / xstd2) - (sin2t / ystd2))
    c = 0.5 * ((sint2 / xstd2) + (cost2 / ystd2))
    return amplitude * np.exp(-((a * xdiff ** 2) + (b * xdiff * ydiff) + (c * ydiff ** 2)))


def fit_deriv(x, y, amplitude, x_mean, y_mean, x_stddev, y_stddev, theta):
    cost = np.cos(theta)
    sint = np.sin(theta)
    cost2 = np.cos(theta) ** 2
    sint2 = np.sin(theta) ** 2
    cos2t = np.cos(2.0 * theta)
    sin2t = np.sin(2.0 * theta)
    xstd2 = x_stddev ** 2
    ystd2 = y_stddev ** 2
    xstd3 = x_stddev ** 3
    ystd3 = y_stddev ** 3
    xdiff = x - x_mean
    ydiff = y - y_mean
    xdiff2 = xdiff ** 2
    ydiff2 = ydiff ** 2
    a = 0.5 * ((cost2 / xstd2) + (sint2 / ystd2))
    b = 0.5 * ((sin2t / xstd2) - (sin2t / ystd2))
    c = 0.5 * ((sint2 / xstd2) + (cost2 / ystd2))
    g = amplitude * np.exp(-((a * xdiff2) + (b * xdiff * ydiff) + (c * ydiff2)))
    da_dtheta = sint * cost * ((1.0 / ystd2) - (1.0 / xstd2))
    da_dx_stddev = -cost2 / xstd3
    da_dy_stddev = -sint2 / ystd3
    db_dtheta = (cos2t / xstd2) - (cos2t / ystd2)
    db_dx_stddev = -sin2t / xstd3
    db_dy_stddev = sin2t / ystd3
    dc_dtheta = -da_dtheta
    dc_dx_stddev = -sint2 / xstd3
    dc_dy_stddev = -cost2 / ystd3
    dg_dA = g / amplitude
    dg_dx_mean = g * ((2.0 * a * xdiff) + (b * ydiff))
    dg_dy_mean = g * ((b * xdiff) + (2.0 * c * ydiff))
    dg_dx_stddev = g * (-(da_dx_stddev * xdiff2 + db_dx_stddev * xdiff * ydiff
                          + dc_dx_stddev * ydiff2))
    dg_dy_stddev = g * (-(da_dy_stddev * xdiff2 + db_dy_stddev * xdiff * ydiff
                          + dc_dy_stddev * ydiff2))
    dg_dtheta = g * (-(da_dtheta * xdiff2 + db_dtheta * xdiff * ydiff + dc_dtheta * ydiff2))
    return [dg_dA, dg_dx_mean, dg_dy_mean, dg_dx_stddev, dg_dy_stddev, dg_dtheta]


def clipped(p):
    """fitter_to_model_params: both standard deviations bounded below."""
    p = np.array(p, dtype=float)
    p[3] = np.fmax(p[3], FLOAT_EPSILON)
    p[4] = np.fmax(p[4], FLOAT_EPSILON)
    return p


# ---- the fit -----------------------------------------------------------------------
def fit_window(z, x0, y0, tight=False, order=None):
    """LevMarLSQFitter on the 15 x 15 window ``z`` whose first pixel is
    (row y0, column x0) of its plane: dict(params [6] with absolute means,
    nfev, ier, converged).  ``order`` permutes the 225 pixels (a check of the
    yardstick's own noise).  Raises ValueError, as the reference's fit does,
    when the window is not 15 x 15 or holds a pixel that is not finite."""
    z = np.asarray(z)
    if z.shape != (WINDOW, WINDOW):
        raise ValueError(f"the window has shape {z.shape}")
    if not np.isfinite(z).all():
        raise ValueError("the window has a pixel that is not finite")
    y, x = np.mgrid[y0:y0 + WINDOW, x0:x0 + WINDOW]
    xr, yr, zr = np.ravel(x), np.ravel(y), np.ravel(z).astype(float)
    if order is not None:
        xr, yr, zr = xr[order], yr[order], zr[order]
    p0 = np.array([np.max(z), np.mean(x), np.mean(y), 1.0, 1.0, 0.0], dtype=float)

    def objective(p):
        return evaluate(xr, yr, *clipped(p)) - zr

    def deriv(p):
        return [np.ravel(d) for d in fit_deriv(xr, yr, *p)]

    if tight:
        stop = dict(maxfev=2000, xtol=1e-14, ftol=1e-14)
    else:
        stop = dict(maxfev=100, xtol=1e-7, ftol=1.49012e-8)
    with np.errstate(all="ignore"):
        p, _, info, _, ier = leastsq(objective, p0, Dfun=deriv, col_deriv=True,
                                     epsfcn=np.sqrt(np.finfo(float).eps), full_output=True,
                                     **stop)
    nfev = int(info["nfev"])
    return dict(params=clipped(p), nfev=nfev, ier=int(ier),
                converged=bool(ier in (1, 2, 3, 4) and nfev < stop["maxfev"]))


def window_origin(pixloc):
    """(x0, y0) of the window about the rounded pixel (x, y)."""
    return int(pixloc[0]) - HALF, int(pixloc[1]) - HALF


def on_plane(x0, y0, ny, nx):
    return 0 <= x0 and x0 + WINDOW <= nx and 0 <= y0 and y0 + WINDOW <= ny


def fit_plane(plane, x0, y0, tight=False):
    return fit_window(np.asarray(plane)[y0:y0 + WINDOW, x0:x0 + WINDOW], x0, y0, tight)


def image_x(im):
    """The "x" coordinate of ska-sdp-datamodels' Image, degrees."""
    w = im.image_acc.wcs.wcs
    nx = int(im["pixels"].data.shape[3])
    cell = abs(w.cdelt[1])
    return np.linspace(w.crval[0] - cell * nx / 2, w.crval[0] + cell * nx / 2, nx, endpoint=False)


def fit_component(im, sc, tight=False, **kwargs):
    """Steps 1-6 for an Image with numpy pixels: dict(fitted, ra, dec, flux,
    shape, params, fit [6] or None).  ``fitted`` False is the reference's
    "return sc": every other field is then the input component's."""
    from ska_sdp_func_python_amd import datamodels as dm
    pixels = np.asarray(im["pixels"].data)
    ny, nx = pixels.shape[2:]
    wcs = im.image_acc.wcs
    px, py = dm.skycoord_to_pixel(sc.direction, wcs, origin=0)
    out = dict(fitted=False, ra=sc.direction.ra.rad, dec=sc.direction.dec.rad,
               flux=np.asarray(sc.flux), shape=sc.shape, params=dict(sc.params), fit=None)
    if not (np.isfinite(px[0]) and np.isfinite(py[0])):
        return out
    pixloc = np.round([px[0], py[0]]).astype("int")
    x0, y0 = window_origin(pixloc)
    if not on_plane(x0, y0, ny, nx):
        return out   # short or empty slices: ValueError in the reference
    try:
        fit = fit_plane(pixels[0, 0], x0, y0, tight)
    except ValueError:
        return out
    p = fit["params"]
    direction = dm.pixel_to_skycoord(p[1], p[2], wcs, 0)
    iy, ix = round(float(p[2])), round(float(p[1]))
    out.update(fitted=True, ra=direction.ra.rad, dec=direction.dec.rad, fit=p)
    if 0 <= iy < ny and 0 <= ix < nx:
        out["flux"] = pixels[:, :, iy, ix]
    x_fwhm, y_fwhm = p[3] * SIGMA_TO_FWHM, p[4] * SIGMA_TO_FWHM
    if kwargs.get("force_point_sources", True) or (x_fwhm <= 0.0 or y_fwhm <= 0.0):
        out["shape"] = "Point"
    else:
        x = image_x(im)
        cellsize = np.abs(x[0] - x[-1]) / len(x)
        if y_fwhm > x_fwhm:
            beam = {"bmaj": np.rad2deg(y_fwhm * cellsize), "bmin": np.rad2deg(x_fwhm * cellsize),
                    "bpa": np.rad2deg(p[5])}
        else:
            beam = {"bmaj": np.rad2deg(x_fwhm * cellsize), "bmin": np.rad2deg(y_fwhm * cellsize),
                    "bpa": np.rad2deg(p[5]) + 90.0}
        out["shape"] = "Gaussian"
        out["params"] = beam
    return out


# ---- stand-in for the kernel wrapper (CPU tensors in place of device ones) ----------
def fake_gauss_fit(planes, x0, y0, max_iter=100, tight=True):
    import torch
    nfit = len(planes)
    params = np.zeros((nfit, 6))
    status = np.zeros(nfit, dtype=np.int32)
    niter = np.zeros(nfit, dtype=np.int32)
    for f, plane in enumerate(planes):
        p = plane.numpy()
        if not on_plane(int(x0[f]), int(y0[f]), *p.shape):
            raise ValueError("gauss_fit: a window does not lie on its plane")
        try:
            fit = fit_plane(p, int(x0[f]), int(y0[f]), tight)
        except ValueError:
            status[f] = 2
            params[f] = np.nan
            continue
        params[f], niter[f] = fit["params"], fit["nfev"]
        status[f] = 0 if fit["converged"] else 1
    return torch.as_tensor(params), torch.as_tensor(status), torch.as_tensor(niter)


@contextlib.contextmanager
def host_kernels(tight=True):
    """Inside, fit_skycomponent(s), find_skycomponents and the Taylor-term
    functions run their own host code with the kernel wrappers replaced by the
    restatements, on CPU tensors."""
    import functools
    import torch
    import findcomp_restatement as fr
    from ska_sdp_func_python_amd import _device, kernels
    swaps = [(_device, "device", lambda: torch.device("cpu")),
             (kernels, "gauss_fit", functools.partial(fake_gauss_fit, tight=tight)),
             (kernels, "segment_image", fr.fake_segment_image),
             (kernels, "segment_peaks", fr.fake_segment_peaks)]
    saved = [getattr(mod, name, None) for mod, name, _ in swaps]
    try:
        for mod, name, new in swaps:
            setattr(mod, name, new)
        yield
    finally:
        for (mod, name, _), old in zip(swaps, saved):
            if old is None:
                delattr(mod, name)
            else:
                setattr(mod, name, old)


# ---- case builders ---------------------------------------------------------------------
def gaussian_window(amplitude, fx, fy, sx, sy, theta, noise=0.0, seed=0):
    """A 15 x 15 window of a Gaussian centred (fx, fy) pixels from the window's
    centre pixel, plus seeded normal noise of ``noise`` times |amplitude|."""
    y, x = np.mgrid[0:WINDOW, 0:WINDOW]
    z = evaluate(x, y, amplitude, HALF + fx, HALF + fy, sx, sy, theta)
    if noise:
        z = z + noise * abs(amplitude) * np.random.default_rng(seed).standard_normal(z.shape)
    return z


# name: (amplitude, fx, fy, sigma_x, sigma_y, theta, noise, seed).  The seeds were
# picked on the CPU so that every case converges in the yardstick and its tight
# centre keeps HALF_PIXEL_MARGIN from a half-integer (make_golden_gaussfit.py
# asserts both).  "beam" is the circular restored-beam case.
WINDOW_CASES = {
    "beam_clean":        (1.0, 0.0, 0.0, 1.5, 1.5, 0.0, 0.0, 0),
    "beam_offset_pp":    (2.5, 0.3, 0.2, 1.5, 1.5, 0.0, 0.0, 0),
    "beam_offset_mm":    (0.7, -0.35, -0.15, 1.5, 1.5, 0.0, 0.0, 0),
    "beam_noisy":        (1.0, 0.2, -0.3, 1.5, 1.5, 0.0, 0.01, 11),
    "beam_noisy_pm":     (3.0, -0.25, 0.3, 1.5, 1.5, 0.0, 0.01, 12),
    "ellipse_pos":       (1.0, 0.1, -0.2, 2.4, 1.4, 0.5, 0.0, 0),
    "ellipse_neg":       (1.0, -0.3, 0.25, 2.2, 1.3, -0.6, 0.0, 0),
    "ellipse_pos_noisy": (2.0, 0.35, 0.1, 2.4, 1.4, 0.4, 0.01, 13),
    "ellipse_neg_noisy": (1.5, -0.1, -0.35, 2.0, 1.2, -0.7, 0.01, 14),
    "ellipse_tall":      (1.0, 0.15, 0.3, 1.3, 2.3, 0.3, 0.01, 15),
    # The reference's start amplitude, max(z), is noise for a negative source, and
    # its first Gauss-Newton step then throws widths and centre by ~ A / max(z):
    # on sources of other shapes than the start's the yardstick itself ends with
    # both widths on their bound or at its evaluation cap.  So the negative cases
    # have the start's shape (sigma 1 on the centre pixel), where that step is
    # small, and noise for max(z) to be positive.
    "negative_faint":    (-2.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.003, 20),
    "negative_noisy":    (-2.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.01, 18),
    "narrow":            (1.0, 0.3, -0.3, 0.9, 0.8, 0.0, 0.01, 17),
    "wide":              (1.0, -0.4, 0.2, 3.0, 2.6, 0.0, 0.01, 18),
}
# the windows' home on a plane: first pixel (x0, y0), up to pixel 4000 in x for a
# third of the cases and in y for another third, so that the planes stay small
WINDOW_HOMES = {name: (((37 * k * k + 11 * k) % 3986, (5 * k) % 23) if k % 3 == 0 else
                       ((7 * k) % 19, (53 * k * k + 7 * k) % 3986) if k % 3 == 1 else
                       ((37 * k) % 211, (53 * k) % 197))
                for k, name in enumerate(WINDOW_CASES)}


def home_plane(name, dtype=np.float64):
    """The case's window at its home on a plane just large enough, with a
    ragged margin of 0 .. 3 pixels behind the window."""
    k = list(WINDOW_CASES).index(name)
    x0, y0 = WINDOW_HOMES[name]
    return placed((y0 + WINDOW + k % 2, x0 + WINDOW + 3 * ((k + 1) % 2)), case_window(name),
                  x0, y0, dtype, seed=k)


def case_window(name):
    a, fx, fy, sx, sy, th, noise, seed = WINDOW_CASES[name]
    return gaussian_window(a, fx, fy, sx, sy, th, noise, seed)


def placed(plane_shape, window, x0, y0, dtype=np.float64, seed=1):
    """A plane of faint seeded noise with ``window`` at first pixel (y0, x0)."""
    plane = 1e-3 * np.random.default_rng(seed).standard_normal(plane_shape)
    plane[y0:y0 + WINDOW, x0:x0 + WINDOW] = window
    return plane.astype(dtype)


# ---- the image case of the fixtures ------------------------------------------------------
IMAGE_SHAPE = (40, 48)
# (x, y, sigma_x, sigma_y, theta): two fitted (one wider in x, one wider in y), one
# whose window leaves the image to the left and one whose window leaves it at the top
IMAGE_SOURCES = [(20.3, 17.8, 2.2, 1.4, 0.4), (33.2, 27.4, 1.3, 2.0, -0.3),
                 (5.0, 20.0, 1.5, 1.5, 0.0), (41.0, 33.0, 1.5, 1.5, 0.0)]


def image_geometry():
    return dict(shape=np.array(IMAGE_SHAPE), nchan=2, pol_frame="stokesIQ", cell_deg=0.001,
                phasecentre_deg=np.array([15.0, -35.0]), frequency=1.0e8, channel_bandwidth=1.0e6)


def image_case(pixels=None):
    """The fixtures' image (2 channels, IQ, 40 x 48, numpy pixels: the sources
    as Gaussians scaled per channel and polarisation, plus 0.5 % seeded noise)
    and its components, one per source, at the pixel nearest to each."""
    import skycomp_restatement as sr
    g = image_geometry()
    ny, nx = IMAGE_SHAPE
    if pixels is None:
        y, x = np.mgrid[0:ny, 0:nx]
        rng = np.random.default_rng(31)
        scale = np.array([[1.0, 0.3], [0.8, -0.2]])
        pixels = 0.005 * rng.standard_normal((2, 2, ny, nx))
        for k, (cx, cy, sx, sy, th) in enumerate(IMAGE_SOURCES):
            pixels += (1.0 + 0.5 * k) * scale[:, :, None, None] * evaluate(x, y, 1.0, cx, cy, sx, sy, th)
    im = sr.make_image(g, pixels=pixels)
    flux = np.array([[[1.0, 0.1], [0.9, 0.2]]] * len(IMAGE_SOURCES)) * (1 + np.arange(len(IMAGE_SOURCES)))[:, None, None]
    comps = sr.components_at(im, [(round(s[0]), round(s[1])) for s in IMAGE_SOURCES], flux)
    return im, comps


def taylor_images(to=None, dtype=np.float64):
    """Five single-channel IQ images of 64 x 64 with six restored components
    (sigma 1.5 pixels, on and off pixel centres) whose Stokes-I fluxes follow a
    spectral index and faint seeded noise; numpy pixels, or ``to(pixels)``."""
    import skycomp_restatement as sr
    ny = nx = 64
    freqs = 1.0e8 + 1.0e7 * np.arange(5)
    sources = [(12.0, 14.0, 3.0, -0.7), (30.3, 12.6, 2.0, -0.5), (50.0, 16.2, 1.5, -1.0),
               (15.4, 44.0, 2.5, 0.2), (33.0, 40.0, 4.0, -0.8), (51.7, 47.3, 1.2, 0.0)]
    y, x = np.mgrid[0:ny, 0:nx]
    rng = np.random.default_rng(77)
    images = []
    for chan, f in enumerate(freqs):
        g = dict(shape=np.array([ny, nx]), nchan=1, pol_frame="stokesIQ", cell_deg=0.001,
                 phasecentre_deg=np.array([15.0, -35.0]), frequency=f, channel_bandwidth=1.0e7)
        pixels = 1e-3 * rng.standard_normal((1, 2, ny, nx))
        for cx, cy, flux, alpha in sources:
            blob = evaluate(x, y, 1.0, cx, cy, 1.5, 1.5, 0.0)
            pixels[0, 0] += flux * (f / freqs[2]) ** alpha * blob
            pixels[0, 1] += 0.1 * flux * blob
        images.append(sr.make_image(g, pixels=pixels.astype(dtype), to=to))
    return images, 0.5 * 1.2


def find_taylor_terms(dirty_list, nmoment=1, reference_frequency=None, tight=True, **kwargs):
    """find_skycomponents_frequency_taylor_terms (reference sky_component/
    taylor_terms.py:83-153) composed from the restatements, for images with
    numpy pixels: moment 0 by the host path of image/taylor_terms.py,
    findcomp_restatement.find on it, fit_component per component and channel
    image, then the package's two host functions."""
    import findcomp_restatement as fr
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.image.taylor_terms import (
        calculate_frequency_taylor_terms_from_image_list)
    from ska_sdp_func_python_amd.sky_component.taylor_terms import (
        interpolate_skycomponents_frequency, transpose_skycomponents_to_channels)
    frequency = np.array([d.frequency[0] for d in dirty_list])
    if reference_frequency is None:
        reference_frequency = frequency[len(frequency) // 2]
    moment0 = calculate_frequency_taylor_terms_from_image_list(
        dirty_list, nmoment=1, reference_frequency=reference_frequency)[0]
    try:
        found = fr.find(moment0, threshold=kwargs.get("component_threshold", np.inf))
    except ValueError:
        return []
    comps = []
    for w in found:
        sc = dm.SkyComponent(dm.SkyCoord(w["ra"], w["dec"]), np.asarray(moment0.frequency.data),
                             w["name"], w["flux"],
                             polarisation_frame=moment0.image_acc.polarisation_frame)
        comp = sc.copy()
        comp.frequency = frequency
        comp.flux = np.array([list(fit_component(d, sc, tight)["flux"][0, :]) for d in dirty_list])
        comps.append(comp)
    return transpose_skycomponents_to_channels(
        interpolate_skycomponents_frequency(comps, nmoment=nmoment,
                                            reference_frequency=reference_frequency))


def axial_ratio(params):
    s = np.abs(np.asarray(params)[..., 3:5])
    return np.max(s, axis=-1) / np.min(s, axis=-1)


def half_pixel_margin(params):
    """The distance of the centre from the nearest half-integer, the smaller of
    the two axes'."""
    c = np.asarray(params)[..., 1:3]
    return np.min(np.abs(c - np.floor(c) - 0.5), axis=-1)


def angle_between(ra0, dec0, ra1, dec1):
    """Angular separation in rad (haversine)."""
    h = np.sin((dec1 - dec0) / 2) ** 2 + np.cos(dec0) * np.cos(dec1) * np.sin((ra1 - ra0) / 2) ** 2
    return 2.0 * np.arcsin(np.sqrt(h))
