"""Builders and the numpy restatement shared by the Taylor-term tests and the
generator of their fixtures (tests/golden/make_golden_taylor.py)."""

import numpy as np

from ska_sdp_func_python_amd import datamodels as dm

NCHAN, NPOL, NY, NX = 5, 2, 17, 13
F0, BW = 1.0e8, 3.0e6
POL_FRAME = "stokesIQ"
EXPLICIT_REFERENCE = 1.045e8
COMP_FREQUENCY = F0 + BW * np.arange(NCHAN)


def make_wcs(f0=F0, bw=BW, ny=NY, nx=NX):
    return dm.WCS(4, ["RA---SIN", "DEC--SIN", "STOKES", "FREQ"],
                  [nx // 2 + 1, ny // 2 + 1, 1.0, 1.0], [-0.001, 0.001, 1.0, bw],
                  [15.0, -45.0, 1.0, f0], ["deg", "deg", "", "Hz"])


def make_cube(pixels, f0=F0, bw=BW, pol_frame=POL_FRAME):
    """Image [nchan, npol, ny, nx] on channels f0 + chan * bw."""
    return dm.Image.constructor(pixels, dm.PolarisationFrame(pol_frame),
                                make_wcs(f0, bw, *pixels.shape[2:]))


def make_list(pixels, f0=F0, bw=BW, pol_frame=POL_FRAME):
    """The channels of a cube as single-channel Images [1, npol, ny, nx]."""
    return [make_cube(pixels[chan:chan + 1], f0 + chan * bw, bw, pol_frame)
            for chan in range(pixels.shape[0])]


def cube_pixels():
    """The fixture's cube: normal deviates with a few zeros of either sign."""
    rng = np.random.default_rng(2024)
    cube = rng.normal(size=(NCHAN, NPOL, NY, NX)) * rng.uniform(0.1, 10.0, (NCHAN, NPOL, 1, 1))
    cube[:, :, 3, 4] = 0.0
    cube[:, 0, 5, 6] = -0.0
    cube[1, 1, 7, 8] = -0.0
    return cube


def weights(frequency, reference_frequency, nmoment):
    """w[chan, k] = ((nu_chan - nu_ref) / nu_ref) ** k, numpy.power as in the product."""
    return np.array([[np.power((f - reference_frequency) / reference_frequency, k)
                      for k in range(nmoment)] for f in frequency])


def mix_loop(w, planes):
    """out[k] = sum_c w[k, c] * planes[c]: every output starts from +0.0 and
    adds float64 products in ascending c, one rounding per product and per sum."""
    out = np.zeros((len(w),) + planes[0].shape)
    for k in range(len(w)):
        for c, plane in enumerate(planes):
            out[k] += np.float64(w[k][c]) * np.asarray(plane, dtype=np.float64)
    return out


def components(pol_frame, seed):
    """Three components on the fixture's five channels."""
    rng = np.random.default_rng(seed)
    npol = dm.PolarisationFrame(pol_frame).npol
    flux = rng.uniform(0.5, 10.0, (3, NCHAN, npol))
    flux[..., 1:] *= rng.uniform(-0.2, 0.2, flux[..., 1:].shape)
    return flux


def make_components(flux, pol_frame, frequency=COMP_FREQUENCY):
    return [dm.SkyComponent(dm.SkyCoord(0.26 + 0.01 * k, -0.78), frequency, f"c{k}", flux[k],
                            polarisation_frame=dm.PolarisationFrame(pol_frame))
            for k in range(len(flux))]
