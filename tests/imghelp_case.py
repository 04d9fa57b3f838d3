"""Input builders shared by the imaging-helper tests and the generator of
their fixtures (tests/golden/make_golden_imghelp.py).  Everything is seeded;
the fixtures hold only what the reference's functions returned for it."""

import numpy as np

from ska_sdp_func_python_amd import datamodels as dm

NCHAN, NPOL, NY, NX = 3, 2, 9, 7
POL_FRAME = "stokesIQ"
CLEAN_BEAM = {"bmaj": 0.1, "bmin": 0.05, "bpa": 12.0}


def make_image(pixels, pol_frame=POL_FRAME, f0=1.0e8, bw=1.0e6, clean_beam=None):
    """A canonical Image [nchan, npol, ny, nx] around the given pixels."""
    ny, nx = pixels.shape[2:]
    wcs = dm.WCS(4, ["RA---SIN", "DEC--SIN", "STOKES", "FREQ"],
                 [nx // 2 + 1, ny // 2 + 1, 1.0, 1.0], [-0.001, 0.001, 1.0, bw],
                 [15.0, -45.0, 1.0, f0], ["deg", "deg", "", "Hz"])
    return dm.Image.constructor(pixels, dm.PolarisationFrame(pol_frame), wcs,
                                clean_beam=clean_beam)


# ---- sum_invert_results ------------------------------------------------------
# name -> (entries, None positions, special)
INVERT_CASES = {
    "one": dict(n=1, none=(), seed=11),
    "three_none": dict(n=3, none=(1,), seed=12),
    "zero_plane": dict(n=3, none=(), seed=13, zero_plane=(1, 0)),
    "negative": dict(n=4, none=(), seed=14, negative=(2, (0, 1))),
}


def invert_case(name):
    """The (pixels, sumwt) pairs of a case, None where the list has None.
    Pixels: normal deviates with -0.0 in every fourth pixel.  ``zero_plane``:
    the weights of that [chan, pol] plane are +1, -1 and 0, which sum to 0,
    and the plane's pixels hold a NaN.  ``negative``: one entry's weight of
    one plane is negative, the plane's sum stays positive."""
    spec = INVERT_CASES[name]
    rng = np.random.default_rng(spec["seed"])
    out = []
    for k in range(spec["n"]):
        pixels = rng.normal(size=(NCHAN, NPOL, NY, NX))
        pixels.reshape(-1)[::4] = -0.0
        sumwt = rng.uniform(0.5, 20.0, (NCHAN, NPOL))
        if "zero_plane" in spec:
            sumwt[spec["zero_plane"]] = (1.0, -1.0, 0.0)[k]
            if k == 1:
                pixels[spec["zero_plane"]][2, 3] = np.nan
        if "negative" in spec and k == spec["negative"][0]:
            sumwt[spec["negative"][1]] = -0.25
        out.append(None if k in spec["none"] else (pixels, sumwt))
    return out


def invert_list(name, convert=lambda a: a):
    """The case as the list sum_invert_results takes; ``convert`` maps the pixels."""
    return [None if e is None else (make_image(convert(e[0]), clean_beam=dict(CLEAN_BEAM)), e[1].copy())
            for e in invert_case(name)]


# ---- Visibilities ------------------------------------------------------------
VIS_KINDS = {
    # frequencies (Hz), channel width, scale of uvw (m), diameters (m)
    "mid": dict(freq=1.30e9 + 2.0e7 * np.arange(5), bw=2.0e7, scale=(3000.0, 2500.0, 120.0),
                diameter=[15.0, 15.0, 13.5, 15.0], seed=21),
    "low": dict(freq=1.0e8 + 1.0e6 * np.arange(3), bw=1.0e6, scale=(20000.0, 18000.0, 900.0),
                diameter=38.0, seed=22),
    "one": dict(freq=np.array([1.5e8]), bw=4.0e6, scale=(800.0, 900.0, 30.0), diameter=38.0,
                seed=23),
}
NT, NB = 3, 6


def make_vis(kind, npol=1, dtype=np.complex128, seed=None, uvw=None, diameter=None):
    spec = VIS_KINDS[kind]
    rng = np.random.default_rng(spec["seed"] if seed is None else seed)
    freq = np.asarray(spec["freq"], dtype=float)
    if uvw is None:
        uvw = rng.normal(size=(NT, NB, 3)) * np.array(spec["scale"])
    shape = (NT, NB, len(freq), npol)
    vis = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)
    frame = {1: "stokesI", 2: "linearnp", 4: "linear"}[npol]
    config = dm.Configuration(kind.upper(),
                              diameter=spec["diameter"] if diameter is None else diameter)
    return dm.Visibility.constructor(
        frequency=freq, channel_bandwidth=np.full(len(freq), spec["bw"]),
        phasecentre=dm.SkyCoord(0.3, -0.7), configuration=config, uvw=uvw,
        time=10.0 * np.arange(NT), vis=vis, baselines=np.array([(0, k + 1) for k in range(NB)]),
        polarisation_frame=dm.PolarisationFrame(frame))


# sum_predict_results: positions of None in a list of 5, seeds of the others
PREDICT_NONE = (0, 2)
PREDICT_LEN = 5


def predict_list(dtype=np.complex128, convert=lambda a: a):
    out = []
    for k in range(PREDICT_LEN):
        if k in PREDICT_NONE:
            out.append(None)
            continue
        v = make_vis("low", npol=4, dtype=dtype, seed=40 + k)
        v["vis"].data = convert(v["vis"].data)
        out.append(v)
    return out


# ---- threshold_list ------------------------------------------------------------
def threshold_images(name):
    """Pixel arrays of the lists the threshold cases use."""
    rng = np.random.default_rng({"cubes": 31, "negative": 32, "single": 33, "summed": 34}[name])
    if name == "cubes":      # three sub-images of 3 channels; the peak is in the second
        out = [rng.normal(size=(3, NPOL, NY, NX)) for _ in range(3)]
        out[1][:, 1, 4, 2] += 7.0
        return out
    if name == "negative":   # the largest magnitude is negative
        out = [rng.normal(size=(3, NPOL, NY, NX)) for _ in range(2)]
        out[0][:, 0, 8, 6] -= 9.0
        return out
    if name == "single":     # one channel: refchan 0
        return [rng.normal(size=(1, NPOL, NY, NX)) for _ in range(2)]
    # "summed": the middle channel is small where the channel sum peaks
    out = [0.01 * rng.normal(size=(3, NPOL, NY, NX))]
    out[0][0, 1, 3, 3] = 5.0
    out[0][1, 1, 3, 3] = 0.0
    out[0][2, 1, 3, 3] = 4.0
    out[0][1, 0, 0, 0] = -1.5
    return out


# name -> (list, threshold, fractional_threshold, use_moment0)
THRESHOLD_CASES = {
    "cubes_moment_frac": ("cubes", 0.0, 0.1, True),
    "cubes_moment_abs": ("cubes", 10.0, 0.1, True),
    "cubes_refchan_frac": ("cubes", 0.0, 0.3, False),
    "cubes_refchan_abs": ("cubes", 4.0, 0.3, False),
    "negative_moment": ("negative", 0.01, 0.2, True),
    "negative_refchan": ("negative", 0.01, 0.2, False),
    "single_moment": ("single", 0.0, 0.5, True),
    "single_refchan": ("single", 0.0, 0.5, False),
    "summed_moment": ("summed", 0.0, 1.0, True),
    "summed_refchan": ("summed", 0.0, 1.0, False),
}


def threshold_list_input(name, convert=lambda a: a):
    return [make_image(convert(p)) for p in threshold_images(name)]


# ---- create_image_from_visibility ------------------------------------------------
# name -> (vis kind, kwargs); "pf:<frame>" stands for a PolarisationFrame
IMAGE_CASES = {
    "default": ("mid", dict(npixel=64)),
    "too_large": ("mid", dict(npixel=32, cellsize=1.0)),
    "no_override": ("mid", dict(npixel=32, cellsize=1.0, override_cellsize=False)),
    "zero_cell": ("mid", dict(npixel=32, cellsize=0.0, override_cellsize=False)),
    "small_cell": ("low", dict(npixel=48, cellsize=1.0e-6)),
    "mfs": ("mid", dict(npixel=32, nchan=1)),
    "all_channels": ("low", dict(npixel=32, nchan=3)),
    "multi_mfs": ("mid", dict(npixel=32, nchan=2)),
    "explicit": ("mid", dict(npixel=32, frequency=[1.1e9, 1.2e9], channel_bandwidth=5.0e7,
                             nchan=1)),
    "polarised": ("low", dict(npixel=16, polarisation_frame="pf:stokesIQUV")),
    "one_channel": ("one", dict(npixel=16)),
}
IMAGE_REFUSED = ("one", dict(nchan=2))


def image_kwargs(kwargs):
    out = dict(kwargs)
    if "frequency" in out:
        out["frequency"] = np.array(out["frequency"])
    if "polarisation_frame" in out:
        out["polarisation_frame"] = dm.PolarisationFrame(out["polarisation_frame"][3:])
    return out


def image_summary(im):
    w = im.image_acc.wcs.wcs
    return dict(shape=np.array(im["pixels"].data.shape), crpix=np.array(w.crpix),
                cdelt=np.array(w.cdelt), crval=np.array(w.crval),
                frame=np.array(im.image_acc.polarisation_frame.type))


# ---- advise_wide_field -----------------------------------------------------------
ADVISE_CASES = {
    "mid_f1": ("mid", dict(facets=1, verbose=False)),
    "mid_f4": ("mid", dict(facets=4, verbose=True)),
    "low_f1": ("low", dict(facets=1, verbose=True, delA=0.05, guard_band_image=3.0)),
    "low_f4": ("low", dict(facets=4, verbose=False, oversampling_synthesised_beam=4.0)),
}

RAD_DEG_ARCSEC_INPUTS = [0.0, 1.0, 4.84813681109536e-06, 0.0123456789, -2.5e-4, 3.0e3]


def recentre_input():
    rng = np.random.default_rng(51)
    return rng.normal(size=(17, 3)) * np.array([2000.0, 1500.0, 90.0]), 0.0123, -0.0045
