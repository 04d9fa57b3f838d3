"""Builders shared by the facet tests and the generator of their fixtures
(tests/golden/make_golden_facets.py)."""

import numpy as np

from ska_sdp_func_python_amd import datamodels as dm

NCHAN, POL_FRAME = 2, "stokesIQ"
F0, BW = 1.0e8, 3.0e6

# (ny, nx, facets, overlap, taper, dtype); the first plants one -0.0 pixel
CASES = {
    "nooverlap": (24, 24, 2, 0, None, "float64"),
    "margins": (50, 50, 4, 0, None, "float64"),
    "linear_nonsquare": (26, 22, 2, 2, "linear", "float64"),
    "quadratic": (24, 24, 2, 2, "quadratic", "float64"),
    "tukey": (24, 24, 2, 3, "tukey", "float64"),
    "flat_overlap": (24, 24, 2, 2, None, "float64"),
    "ninefold": (30, 30, 3, 3, "linear", "float64"),
    "sixteenfold": (40, 40, 4, 4, "linear", "float64"),
    "linear_f32": (24, 24, 2, 2, "linear", "float32"),
}
MINUS_ZERO = {"nooverlap": (1, 0, 5, 7)}
# rasters that the reference itself refuses: (ny, nx, facets, overlap)
REFUSED = [(27, 27, 3, 0), (24, 24, 2, 12)]


def make_wcs(ny, nx, f0=F0, bw=BW):
    return dm.WCS(4, ["RA---SIN", "DEC--SIN", "STOKES", "FREQ"],
                  [nx // 2 + 1, ny // 2 + 1, 1.0, 1.0], [-0.001, 0.001, 1.0, bw],
                  [15.0, -45.0, 1.0, f0], ["deg", "deg", "", "Hz"])


def make_image(pixels, pol_frame=POL_FRAME):
    """Image [nchan, npol, ny, nx] of numpy or device pixels."""
    return dm.Image.constructor(pixels, dm.PolarisationFrame(pol_frame),
                                make_wcs(*pixels.shape[2:]))


def image_pixels(ny, nx, dtype="float64", seed=0, nchan=NCHAN, npol=2):
    rng = np.random.default_rng(1000 * ny + nx + seed)
    return rng.normal(size=(nchan, npol, ny, nx)).astype(dtype)


def case_pixels(name):
    ny, nx, facets, overlap, taper, dtype = CASES[name]
    pixels = image_pixels(ny, nx, dtype, seed=len(name))
    if name in MINUS_ZERO:
        pixels[MINUS_ZERO[name]] = -0.0
    return pixels


def facet_pixels(views):
    """Facet i is view i times (1 + 0.1 i), a copy: a wrong order or a wrong
    facet shows in the gather.  ``views`` are the numpy pixels of scattered
    facets."""
    return [v * v.dtype.type(1 + 0.1 * i) for i, v in enumerate(views)]


def facet_images(subimages):
    scaled = facet_pixels([s["pixels"].data for s in subimages])
    return [dm.Image.constructor(p, s.image_acc.polarisation_frame, s.image_acc.wcs)
            for p, s in zip(scaled, subimages)]
