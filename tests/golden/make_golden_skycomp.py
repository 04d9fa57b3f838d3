"""Generate the sky-component image fixtures tests/golden/skycomp_*.npz from the
REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_skycomp.py

The reference's insert_skycomponent, restore_skycomponent,
voronoi_decomposition and image_voronoi_iter (sky_component/operations.py
:583-815), insert_array and the three insert functions
(util/array_functions.py:102-178), grdsf (fourier_transforms/
fft_coordinates.py) and convert_clean_beam_to_pixels (image/operations.py
:58-75) are AST-extracted and executed with numpy on the datamodels shim, as
make_golden.py does.  Only inputs and outputs are stored -- no reference
source text.

astropy is absent, so three stand-ins are supplied: ``u.rad`` (a unit that
leaves numbers as they are), ``SkyCoord(ras, decs)`` (a list of the shim's
SkyCoord, which the shim's skycoord_to_pixel takes) and ``models.Gaussian2D``.
The last is written from astropy's definition,
    a = (cos^2 t / sx^2 + sin^2 t / sy^2) / 2
    b = (sin 2t / sx^2 - sin 2t / sy^2) / 2
    c = (sin^2 t / sx^2 + cos^2 t / sy^2) / 2
    g = amplitude exp(-(a dx^2 + b dx dy + c dy^2)),
so THE RESTORE FIXTURES ARE FAITHFUL TO THE REFERENCE ONLY AS FAR AS THAT
STAND-IN IS.

Images are 83 rows x 61 columns (non-square, no multiple of a tile), built
with Image.constructor and a SIN WCS about (ra, dec) = (0, 0), where the
projection is exact enough for a component to sit on a half pixel exactly;
they start from skycomp_restatement.start_pixels, not from zero.  Components
are stored as directions (radians), frequencies and fluxes.

  skycomp_taps.npz            the three insert functions on a set of arguments
  skycomp_insert_<method>.npz Nearest / Sinc / Lanczos / PSWF: 3-chan IQUV, 12
                              components on 4 frequencies: two on one pixel,
                              overlapping windows, windows flush with each
                              border, fractional parts of exactly .5, no
                              integer positions
  skycomp_insert_lanczos_bw.npz  bandwidth 0.5: windows of 32 pixels
  skycomp_insert_freq5.npz    components on 5 frequencies
  skycomp_insert_nearest_off.npz  one component off the image, one behind the
                              tangent plane
  skycomp_insert_single.npz   stokesI, 1 channel, one bare component
  skycomp_restore_single.npz  stokesI, 1 channel, one bare component, circular beam
  skycomp_restore_iquv.npz    3-chan IQUV, 8 components between pixels, beam
                              bmaj != bmin, bpa = -60; one centre 10 pixels
                              off the image
  skycomp_restore_freq5.npz   components on 5 frequencies
  skycomp_voronoi.npz         9 components: label image, pixels per region
"""

import collections
import math
import os
import sys
import types
from typing import List, Union

import numpy as np
from scipy import interpolate
from scipy.spatial import Voronoi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import dm, load_reference, save  # noqa: E402

import skycomp_restatement as R  # noqa: E402

NY, NX = R.NY, R.NX
CELL_DEG = 0.001
FREQ0, BW = 1.0e8, 1.0e6


# ---- astropy stand-ins -------------------------------------------------------
class _Rad:
    def __rmul__(self, other):
        return np.asarray(other, dtype=float)

    __mul__ = __rmul__


def _skycoord(ras, decs, frame="icrs"):
    return [dm.SkyCoord(float(ra), float(dec)) for ra, dec in zip(ras, decs)]


class _Gaussian2D:
    def __init__(self, amplitude, x_mean, y_mean, x_stddev, y_stddev, theta):
        self.p = (amplitude, x_mean, y_mean, x_stddev, y_stddev, theta)

    def __call__(self, x, y):
        amplitude, x_mean, y_mean, x_stddev, y_stddev, theta = self.p
        cost2 = np.cos(theta) ** 2
        sint2 = np.sin(theta) ** 2
        sin2t = np.sin(2.0 * theta)
        xstd2 = x_stddev**2
        ystd2 = y_stddev**2
        xdiff = x - x_mean
        ydiff = y - y_mean
        a = 0.5 * ((cost2 / xstd2) + (sint2 / ystd2))
        b = 0.5 * ((sin2t / xstd2) - (sin2t / ystd2))
        c = 0.5 * ((sint2 / xstd2) + (cost2 / ystd2))
        return amplitude * np.exp(-((a * xdiff**2) + (b * xdiff * ydiff) + (c * ydiff**2)))


def _reference():
    fc = load_reference("fourier_transforms/fft_coordinates.py", ["grdsf"])
    af = load_reference("util/array_functions.py",
                        ["insert_function_sinc", "insert_function_L", "insert_function_pswf",
                         "insert_array"], {"grdsf": fc["grdsf"]})
    imops = load_reference("image/operations.py", ["convert_clean_beam_to_pixels"])
    ops = load_reference(
        "sky_component/operations.py",
        ["insert_skycomponent", "restore_skycomponent", "voronoi_decomposition",
         "image_voronoi_iter"],
        {"collections": collections, "Union": Union, "List": List, "SkyComponent": dm.SkyComponent,
         "u": types.SimpleNamespace(rad=_Rad()), "SkyCoord": _skycoord,
         "skycoord_to_pixel": dm.skycoord_to_pixel, "interpolate": interpolate,
         "insert_array": af["insert_array"], "insert_function_L": af["insert_function_L"],
         "insert_function_sinc": af["insert_function_sinc"],
         "insert_function_pswf": af["insert_function_pswf"],
         "convert_clean_beam_to_pixels": imops["convert_clean_beam_to_pixels"],
         "models": types.SimpleNamespace(Gaussian2D=_Gaussian2D), "Voronoi": Voronoi})
    return af, ops


# ---- components ----------------------------------------------------------------
def _ref_component(ra, dec, frequency, flux):
    """What the reference reads of a SkyComponent (astropy's .radian included)."""
    angle = lambda v: types.SimpleNamespace(rad=float(v), radian=float(v))
    return types.SimpleNamespace(direction=types.SimpleNamespace(ra=angle(ra), dec=angle(dec)),
                                 frequency=types.SimpleNamespace(data=np.asarray(frequency, float)),
                                 flux=np.asarray(flux), shape="Point")


def _direction(wcs, x, y, exact):
    """(ra, dec) in radians of the 0-based pixel (x, y); with ``exact`` the
    direction is moved by a few ulps until it projects to (x, y) exactly."""
    d = dm.pixel_to_skycoord(x, y, wcs, origin=0)
    ra, dec = d.ra.rad, d.dec.rad
    if not exact:
        return ra, dec
    pix = lambda ra_, dec_: [float(v[0]) for v in dm.skycoord_to_pixel(dm.SkyCoord(ra_, dec_), wcs, origin=0)]
    for sd in sorted(range(-300, 301), key=abs):
        dec_t = dec
        for _ in range(abs(sd)):
            dec_t = math.nextafter(dec_t, math.inf if sd > 0 else -math.inf)
        if pix(ra, dec_t)[1] != y:
            continue
        for sr in sorted(range(-300, 301), key=abs):
            ra_t = ra
            for _ in range(abs(sr)):
                ra_t = math.nextafter(ra_t, math.inf if sr > 0 else -math.inf)
            if pix(ra_t, dec_t) == [x, y]:
                return ra_t, dec_t
    raise AssertionError(f"no direction projects to ({x}, {y}) exactly")


def _geometry(nchan, pol_frame):
    return dict(shape=np.array([NY, NX]), nchan=np.array(nchan), pol_frame=np.array(pol_frame),
                cell_deg=np.array(CELL_DEG), phasecentre_deg=np.array([0.0, 0.0]),
                frequency=np.array(FREQ0), channel_bandwidth=np.array(BW))


def _case(nchan, pol_frame, positions, comp_frequency, rng, exact=(), extra_radec=()):
    """The fixture's inputs, the Image and the components as the reference reads them."""
    g = _geometry(nchan, pol_frame)
    im = R.make_image(g)
    wcs = im.image_acc.wcs
    radec = [_direction(wcs, x, y, k in exact) for k, (x, y) in enumerate(positions)]
    radec += list(extra_radec)
    npol = dm.PolarisationFrame(pol_frame).npol
    flux = rng.uniform(0.5, 10.0, (len(radec), len(comp_frequency), npol))
    flux[..., 1:] *= rng.uniform(-0.2, 0.2, flux[..., 1:].shape)
    g.update(comp_radec_rad=np.array(radec), comp_frequency=np.asarray(comp_frequency, float),
             comp_flux=flux, single=np.array(0))
    comps = [_ref_component(ra, dec, comp_frequency, flux[k]) for k, (ra, dec) in enumerate(radec)]
    return g, im, comps


POSITIONS = [(20.3, 30.7), (20.4, 30.6), (27.2, 36.4), (10.5, 50.3), (11.5, 60.5), (30.6, 8.2),
             (30.4, 74.8), (8.3, 40.6), (52.7, 41.4), (8.4, 8.4), (45.35, 20.65), (40.8, 66.2)]
EXACT = (3, 4)
IMAGE_FREQ = FREQ0 + BW * np.arange(3)
FREQ4 = FREQ0 + BW * np.array([-0.5, 0.4, 1.3, 2.5])
FREQ5 = FREQ0 + BW * np.array([-0.25, 0.5, 1.0, 1.75, 2.25])


def make_taps(af):
    x = np.concatenate([np.arange(-8, 8) - 0.3, np.arange(-8, 8) + 0.5, 0.5 * (np.arange(-16, 16) - 0.45),
                        np.array([0.0, -0.0, 1.0, -5.0, 5.0, 3.75, 4.999, 1e-9])])
    save("skycomp_taps.npz", x=x, sinc=af["insert_function_sinc"](x), lanczos=af["insert_function_L"](x),
         pswf=af["insert_function_pswf"](x))


def make_insert(ops):
    wcs = R.make_image(_geometry(3, "stokesIQUV")).image_acc.wcs
    pix = dm.skycoord_to_pixel([dm.SkyCoord(*_direction(wcs, x, y, k in EXACT))
                                for k, (x, y) in enumerate(POSITIONS)], wcs, origin=0)
    assert pix[0][3] == 10.5 and pix[0][4] == 11.5 and pix[1][4] == 60.5
    assert not np.any(pix[0] == np.round(pix[0])) and not np.any(pix[1] == np.round(pix[1]))
    ix, iy = np.round(pix[0]).astype(int), np.round(pix[1]).astype(int)
    assert ix[3] == 10 and ix[4] == 12 and (ix[0], iy[0]) == (ix[1], iy[1])
    assert (iy - 8).min() == 0 and (iy + 8).max() == NY and (ix - 8).min() == 0 and (ix + 8).max() == NX
    for seed, (tag, method) in enumerate([("nearest", "Nearest"), ("sinc", "Sinc"),
                                          ("lanczos", "Lanczos"), ("pswf", "PSWF")]):
        g, im, comps = _case(3, "stokesIQUV", POSITIONS, FREQ4, np.random.default_rng(40 + seed), EXACT)
        assert ops["insert_skycomponent"](im, comps, insert_method=method) is im
        save(f"skycomp_insert_{tag}.npz", method=np.array(method), bandwidth=np.array(1.0),
             support=np.array(8), out_pixels=im["pixels"].data, **g)
    # bandwidth 0.5: windows of 32, flush with the borders at (16, 16) and (45, 67)
    pos = [(20.3, 30.7), (20.4, 30.6), (16.3, 16.4), (44.7, 66.8), (30.5, 40.25)]
    g, im, comps = _case(3, "stokesIQUV", pos, FREQ4, np.random.default_rng(50), exact=(4,))
    ops["insert_skycomponent"](im, comps, insert_method="Lanczos", bandwidth=0.5, support=8)
    save("skycomp_insert_lanczos_bw.npz", method=np.array("Lanczos"), bandwidth=np.array(0.5),
         support=np.array(8), out_pixels=im["pixels"].data, **g)
    g, im, comps = _case(3, "stokesIQUV", POSITIONS[:4], FREQ5, np.random.default_rng(51))
    ops["insert_skycomponent"](im, comps, insert_method="Lanczos")
    save("skycomp_insert_freq5.npz", method=np.array("Lanczos"), bandwidth=np.array(1.0),
         support=np.array(8), out_pixels=im["pixels"].data, **g)
    # Nearest: pixel (70.2, 30.1) is off the image, ra = pi is behind the tangent plane
    g, im, comps = _case(3, "stokesIQUV", POSITIONS[:3] + [(70.2, 30.1)] + POSITIONS[3:5], FREQ4,
                         np.random.default_rng(52), exact=(4, 5), extra_radec=[(math.pi, 0.1)])
    with np.errstate(invalid="ignore"):
        ops["insert_skycomponent"](im, comps, insert_method="Nearest")
    save("skycomp_insert_nearest_off.npz", method=np.array("Nearest"), bandwidth=np.array(1.0),
         support=np.array(8), out_pixels=im["pixels"].data, nbad=np.array(2), **g)
    g, im, comps = _case(1, "stokesI", [(33.3, 47.6)], IMAGE_FREQ[:1], np.random.default_rng(53))
    g["single"] = np.array(1)
    assert ops["insert_skycomponent"](im, comps[0], insert_method="Lanczos") is im
    save("skycomp_insert_single.npz", method=np.array("Lanczos"), bandwidth=np.array(1.0),
         support=np.array(8), out_pixels=im["pixels"].data, **g)


def make_restore(ops):
    def beam(bmaj_pix, bmin_pix, bpa):
        return {"bmaj": bmaj_pix * CELL_DEG, "bmin": bmin_pix * CELL_DEG, "bpa": bpa}

    def store(tag, g, im, clean_beam):
        assert im.attrs["clean_beam"] == clean_beam
        save(f"skycomp_restore_{tag}.npz", out_pixels=im["pixels"].data,
             clean_beam=np.array([clean_beam["bmaj"], clean_beam["bmin"], clean_beam["bpa"]]), **g)

    g, im, comps = _case(1, "stokesI", [(33.3, 47.6)], IMAGE_FREQ[:1], np.random.default_rng(60))
    g["single"] = np.array(1)
    cb = beam(4.0, 4.0, 0.0)
    assert ops["restore_skycomponent"](im, comps[0], clean_beam=cb) is im
    store("single", g, im, cb)
    pos = [(20.3, 30.7), (20.4, 30.6), (27.2, 36.4), (-10.4, 40.3), (52.7, 41.4), (8.4, 8.4),
           (45.35, 76.65), (40.8, 66.2)]
    g, im, comps = _case(3, "stokesIQUV", pos, IMAGE_FREQ, np.random.default_rng(61))
    cb = beam(6.0, 3.5, -60.0)
    ops["restore_skycomponent"](im, comps, clean_beam=cb)
    store("iquv", g, im, cb)
    g, im, comps = _case(3, "stokesIQUV", pos[:2] + pos[4:5], FREQ5, np.random.default_rng(62))
    ops["restore_skycomponent"](im, comps, clean_beam=cb)
    store("freq5", g, im, cb)


def make_voronoi(ops):
    rng = np.random.default_rng(70)
    pos = np.stack([rng.uniform(2, NX - 2, 9), rng.uniform(2, NY - 2, 9)], 1)
    g, im, comps = _case(1, "stokesI", [tuple(p) for p in pos], IMAGE_FREQ[:1], rng)
    vor, labels = ops["voronoi_decomposition"](im, comps)
    # no near ties: at every pixel the two smallest distances differ by > 1e-9
    j, i = np.indices((NY, NX))
    d = np.sort(np.hypot(j[..., None] - vor.points[:, 1], i[..., None] - vor.points[:, 0]), axis=-1)
    assert (d[..., 1] - d[..., 0]).min() > 1e-9
    masks = list(ops["image_voronoi_iter"](im, comps))
    assert len(masks) == labels.max() + 1 == 9
    counts = np.array([int(m["pixels"].data[0, 0].sum()) for m in masks])
    assert counts.sum() == NY * NX and all(m["pixels"].data.shape == (1, 1, NY, NX) for m in masks)
    one = list(ops["image_voronoi_iter"](im, comps[:1]))
    assert len(one) == 1 and np.all(one[0]["pixels"].data == 1.0)
    save("skycomp_voronoi.npz", labels=labels, region_counts=counts, points=vor.points, **g)


def main():
    af, ops = _reference()
    make_taps(af)
    make_insert(ops)
    make_restore(ops)
    make_voronoi(ops)


if __name__ == "__main__":
    main()
