"""Generate the multi-scale multi-frequency CLEAN golden fixtures
tests/golden/mfsclean_*.npz from the REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_mfsclean.py

The reference's msmfsclean and its helpers (image/cleaners.py:686-1157), the
two image-list Taylor-term functions (image/taylor_terms.py:160-288) and
mmclean_kernel_list with find_window_list and common_arguments
(image/deconvolution.py) are AST-extracted and executed with numpy, as
make_golden.py does.  Only inputs and outputs are stored -- no reference
source text.

Fixtures:
  mfsclean_inputs.npz     the shared dirty and PSF moments, window, sensitivity
  mfsclean_<case>.npz     model, residual and the settings of one case
                          (F1..F11); the *_key entries name its arrays in
                          mfsclean_inputs.npz, of which the case takes the
                          first nmoment dirty and 2 * nmoment (1) PSF moments
  mfsclean_L1_inputs.npz  the 7-channel, 2-polarisation dirty and PSF cubes
  mfsclean_L1.npz         mmclean_kernel_list on them: component and residual
                          cubes, the cleaned moments they were rebuilt from
                          and the dirty and PSF moments of the inputs

Inputs: 7 channels, 100 .. 160 MHz.  The PSF of a channel is the mean of 300
random cosines whose uv scale with the channel's frequency, so that the PSF
moments are not multiples of one another; the dirty image is that PSF laid
down at a dozen sources of either sign with spectral indices in [-1.5, 0.5],
three of them on (0, 0), (ny - 1, nx - 2) and (1, nx - 1), plus 0.02 rms
noise per channel.  The moments are formed by the reference's
calculate_image_list_frequency_moments and divided by the peak of the PSF
moments, as mmclean_kernel_list does.

Gap condition: at every iteration of every case the relative gap between
the best and the second-best value is >= 1e-9 within each scale's unweighted
search and between the scales' weighted maxima, and |mval[0]| differs from
the stopping threshold by >= 1e-9 relative, so that no golden rests on a
near-tie that another summation order could flip.  F4 must choose at least
one pixel where its scale's window is 0 (the window chooses the scale, not
the pixel), F10 must stop on its threshold before niter / 2.  A seed that
misses any of this is skipped and the next one tried.
"""

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import dm, load_reference, save  # noqa: E402

MIN_GAP = 1e-9
NCHAN = 7
F0, BW = 1.0e8, 1.0e7
CLEANER_DEFS = ["overlapIndices", "argmax", "create_scalestack", "convolve_scalestack",
                "convolve_convolve_scalestack", "spheroidal_function", "msmfsclean",
                "find_global_optimum", "update_scale_moment_residual", "update_moment_model",
                "calculate_scale_moment_residual", "calculate_scale_scale_moment_moment_psf",
                "calculate_scale_inverse_moment_moment_hessian",
                "calculate_scale_moment_principal_solution", "find_optimum_scale_zero_moment"]
TAYLOR_DEFS = ["calculate_image_list_frequency_moments",
               "calculate_image_list_from_frequency_taylor_terms"]
LIST_DEFS = ["mmclean_kernel_list", "common_arguments", "find_window_list"]


class Rejected(Exception):
    pass


def _gap(values):
    """Relative gap between the largest |value| and the runner-up."""
    flat = np.abs(np.asarray(values, dtype=float)).ravel()
    if flat.size < 2:
        return np.inf
    i = int(flat.argmax())
    best = flat[i]
    if not best > 0.0:
        return np.inf
    return (best - np.delete(flat, i).max()) / best


def reference_cleaner(thresh, fracthresh, log):
    """The reference's cleaners namespace with the search and the stop test
    instrumented: ``log`` collects "gaps", "picks" and "outside_window"."""
    ns = load_reference("image/cleaners.py", CLEANER_DEFS, {"time": time})
    find_scale = ns["find_optimum_scale_zero_moment"]
    find_global = ns["find_global_optimum"]
    log.update(gaps=[], picks=[], outside_window=0, absthresh=None)

    def find_scale_and_check(smpsol, sensitivity, windowstack):
        weighted = []
        for s in range(smpsol.shape[0]):
            log["gaps"].append(_gap(smpsol[s, 0]))
            resid = smpsol[s, 0] if windowstack is None else smpsol[s, 0] * windowstack[s]
            if sensitivity is not None:
                resid = sensitivity * resid
            weighted.append(np.abs(resid).max())
        log["gaps"].append(_gap(weighted))
        sx, sy, sscale = find_scale(smpsol, sensitivity, windowstack)
        if windowstack is not None and windowstack[sscale, sx, sy] == 0.0:
            log["outside_window"] += 1
        return sx, sy, sscale

    def find_global_and_check(hsmmpsf, ihsmmpsf, smresidual, windowstack, sensitivity, findpeak):
        if log["absthresh"] is None:
            log["absthresh"] = max(thresh, fracthresh * np.max(np.abs(smresidual[0, 0])))
        out = find_global(hsmmpsf, ihsmmpsf, smresidual, windowstack, sensitivity, findpeak)
        peak = np.fabs(out[3][0])
        log["gaps"].append(abs(peak - log["absthresh"]) / log["absthresh"])
        log["picks"].append((int(out[0]), int(out[1]), int(out[2]), bool(peak < log["absthresh"])))
        return out

    ns["find_optimum_scale_zero_moment"] = find_scale_and_check
    ns["find_global_optimum"] = find_global_and_check
    return ns


def _checked(log):
    gap = min(log["gaps"])
    if gap < MIN_GAP:
        raise Rejected(f"near-tie, gap {gap:.2e}")
    return gap


def _channel_image(data, chan):
    """Single-channel Image [1, npol, ny, nx] of channel ``chan``."""
    im = dm.create_image(max(data.shape[2:]), 0.001, dm.SkyCoord(0.2, -0.7),
                         frequency=F0 + chan * BW, channel_bandwidth=BW)
    im["pixels"].data = data
    if data.shape[1] == 2:
        im.attrs["_polarisation_frame"] = "stokesIQ"
    return im


def _image_list(cube):
    """[nchan, ny, nx] or [nchan, npol, ny, nx] -> list of single-channel Images"""
    if cube.ndim == 3:
        cube = cube[:, None]
    return [_channel_image(cube[chan:chan + 1].copy(), chan) for chan in range(cube.shape[0])]


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    uv = rng.normal(0.0, 0.12, (300, 2))
    freqs = F0 + BW * np.arange(NCHAN)
    scale = freqs / freqs[NCHAN // 2]
    taylor = load_reference("image/taylor_terms.py", TAYLOR_DEFS, {"List": list})
    moments_of = taylor["calculate_image_list_frequency_moments"]

    def psf_at(dy, dx, f):
        """The PSF of relative frequency f at offsets (dy, dx) from its peak."""
        phase = 2.0 * np.pi * f * (uv[:, 0, None, None] * dx + uv[:, 1, None, None] * dy)
        return np.cos(phase).mean(axis=0)

    def psf_cube(pny, pnx):
        dy, dx = np.mgrid[0:pny, 0:pnx]
        return np.array([psf_at(dy - pny // 2, dx - pnx // 2, f) for f in scale])

    def dirty_cube(ny, nx):
        pos = [(0, 0), (ny - 1, nx - 2), (1, nx - 1)]
        pos += [(int(rng.integers(0, ny)), int(rng.integers(0, nx))) for _ in range(9)]
        flux = rng.uniform(0.3, 1.0, len(pos)) * rng.choice([-1.0, 1.0], len(pos), p=[0.3, 0.7])
        alpha = rng.uniform(-1.5, 0.5, len(pos))
        y, x = np.mgrid[0:ny, 0:nx]
        cube = rng.normal(0.0, 0.02, (NCHAN, ny, nx))
        for chan, f in enumerate(scale):
            for (py, px), fl, a in zip(pos, flux, alpha):
                cube[chan] += fl * f ** a * psf_at(y - py, x - px, f)
        return cube

    def moments(dirty, psf, nmoment):
        """As mmclean_kernel_list: 2 * nmoment PSF moments, both over their peak."""
        d = moments_of(_image_list(dirty), nmoment=nmoment)["pixels"].data[:, 0]
        p = moments_of(_image_list(psf), nmoment=2 * nmoment if nmoment > 1 else 1)["pixels"].data[:, 0]
        peak = np.max(p)
        return d / peak, p / peak

    inp = {}
    cubes = {"a": (dirty_cube(96, 80), psf_cube(96, 80)), "b": (dirty_cube(67, 45), psf_cube(33, 33)),
             "c": (dirty_cube(130, 70), psf_cube(40, 64))}
    cubes["a24"] = (cubes["a"][0], cubes["a"][1][:, 48 - 12:48 + 12, 40 - 12:40 + 12].copy())
    for key, nmoment in (("a", 3), ("a24", 3), ("b", 2), ("c", 2)):
        d, p = moments(*cubes[key], nmoment)
        # fewer moments are the leading ones: the peak is moment 0's, whatever their number
        for fewer in range(1, nmoment):
            d2, p2 = moments(*cubes[key], fewer)
            assert np.array_equal(d2, d[:fewer]) and np.array_equal(p2, p[:len(p2)])
        if key != "a24":
            inp[f"dirty_{key}"] = d
        inp[f"psf_{key}"] = p
    window = np.zeros((96, 80))
    window[17:80, 17:64] = rng.uniform(0.5, 1.0, (63, 47))
    inp["window_a"] = window
    y, x = np.mgrid[0:96, 0:80]
    inp["sens_a"] = np.array([
        0.3 + 0.7 * np.exp(-((y - 50.0) ** 2 + (x - 35.0) ** 2) / (2 * 40.0 ** 2)),
        -0.9 * np.exp(-((y - 20.0) ** 2 + (x - 60.0) ** 2) / (2 * 25.0 ** 2))])
    assert (np.abs(inp["sens_a"][1]) > inp["sens_a"][0]).any()  # the maximum over moments matters
    return inp


# case: (dirty, psf, nmoment, window, sens, niter, fracthresh, scales, findpeak)
CASES = {
    "F1": ("dirty_a", "psf_a", 3, None, None, 40, 0.05, [0, 3, 10], "RASCIL"),
    "F2": ("dirty_a", "psf_a", 2, None, None, 40, 0.05, [0, 3, 10], "CASA"),
    "F3": ("dirty_a", "psf_a", 1, None, None, 40, 0.05, [0, 3, 10], "RASCIL"),
    "F4": ("dirty_a", "psf_a", 3, "window_a", None, 40, 0.05, [0, 3, 10], "RASCIL"),
    "F5": ("dirty_a", "psf_a", 2, None, "sens_a", 40, 0.05, [0, 3, 10], "RASCIL"),
    "F6": ("dirty_b", "psf_b", 2, None, None, 40, 0.05, [0, 3, 6], "RASCIL"),
    "F7": ("dirty_a", "psf_a24", 3, None, None, 40, 0.05, [0, 3, 10], "RASCIL"),
    "F8": ("dirty_c", "psf_c", 2, None, None, 40, 0.05, [0, 3, 10], "RASCIL"),
    "F9": ("dirty_a", "psf_a", 3, None, None, 40, 0.05, [0], "RASCIL"),
    "F10": ("dirty_a", "psf_a", 3, None, None, 40, 0.3, [0, 3, 10], "RASCIL"),
    "F11": ("dirty_a", "psf_a", 3, None, None, 1, 0.05, [0, 3, 10], "RASCIL"),
}
GAIN, THRESH = 0.7, 0.0


def make_cases(inp):
    out = {}
    for name, (dk, pk, nmoment, wk, sk, niter, fracthresh, scales, findpeak) in CASES.items():
        dirty = inp[dk][:nmoment].copy()
        psf = inp[pk][:2 * nmoment if nmoment > 1 else 1].copy()
        window = None if wk is None else inp[wk]
        sens = None if sk is None else inp[sk]
        log = {}
        ns = reference_cleaner(THRESH, fracthresh, log)
        t0 = time.time()
        model, res = ns["msmfsclean"](dirty, psf, window, sens, GAIN, THRESH, niter, scales,
                                      fracthresh, findpeak)
        gap = _checked(log)
        picks = log["picks"]
        if name == "F4" and not log["outside_window"]:
            raise Rejected("F4 never chose a pixel outside its scale's window")
        if name == "F10" and not (picks[-1][3] and len(picks) < niter // 2):
            raise Rejected(f"F10 ran {len(picks)} cycles without stopping on its threshold early")
        print(f"{name}: {len(picks)} cycles, scales used {sorted({p[0] for p in picks})}, "
              f"{log['outside_window']} picks outside the window, min gap {gap:.2e}, "
              f"{time.time() - t0:.2f} s")
        out[name] = dict(model=np.asarray(model), residual=np.asarray(res), dirty_key=dk, psf_key=pk,
                         nmoment=nmoment, window_key=wk or "", sens_key=sk or "", gain=GAIN,
                         thresh=THRESH, niter=niter, fracthresh=fracthresh,
                         scales=np.array(scales, dtype=float), findpeak=findpeak, min_gap=gap)
    return out


def make_list_case(seed):
    """L1: mmclean_kernel_list on a 7-channel, 2-polarisation 64 x 48 list,
    nmoment 2, the "quarter" window; the PSF planes of polarisation 1 are
    zero and it is still cleaned, with polarisation 0's PSF."""
    rng = np.random.default_rng(1000 + seed)
    uv = rng.normal(0.0, 0.12, (200, 2))
    scale = (F0 + BW * np.arange(NCHAN)) / (F0 + BW * (NCHAN // 2))
    ny, nx = 64, 48
    y, x = np.mgrid[0:ny, 0:nx]

    def beam(dy, dx, f):
        return np.cos(2 * np.pi * f * (uv[:, 0, None, None] * dx + uv[:, 1, None, None] * dy)).mean(0)

    psf = np.zeros((NCHAN, 2, ny, nx))
    dirty = rng.normal(0.0, 0.02, (NCHAN, 2, ny, nx))
    for pol in range(2):
        pos = [(int(rng.integers(18, 46)), int(rng.integers(14, 34))) for _ in range(5)]
        flux = rng.uniform(0.3, 1.0, 5)
        alpha = rng.uniform(-1.5, 0.5, 5)
        for chan, f in enumerate(scale):
            for (py, px), fl, a in zip(pos, flux, alpha):
                dirty[chan, pol] += fl * f ** a * beam(y - py, x - px, f)
    for chan, f in enumerate(scale):
        psf[chan, 0] = beam(y - ny // 2, x - nx // 2, f)

    log = {}
    kwargs = dict(nmoment=2, niter=30, gain=0.7, fractional_threshold=0.05, scales=[0, 3, 10],
                  threshold=0.0)
    cleaner = reference_cleaner(kwargs["threshold"], kwargs["fractional_threshold"], log)
    taylor = load_reference("image/taylor_terms.py", TAYLOR_DEFS, {"List": list})
    gaps, counts = [], []

    def msmfsclean(*args):
        log["absthresh"] = None  # each polarisation has its own threshold
        out = cleaner["msmfsclean"](*args)
        gaps.append(_checked(log))
        counts.append(len(log["picks"]))
        log["gaps"], log["picks"] = [], []
        return out

    cleaned_moments = []  # the component, then the residual moments, as they are turned into lists

    def from_taylor_terms(im_list, moment_image):
        cleaned_moments.append(moment_image["pixels"].data.copy())
        return taylor[TAYLOR_DEFS[1]](im_list, moment_image)

    ns = load_reference("image/deconvolution.py", LIST_DEFS,
                        {"msmfsclean": msmfsclean, "List": list, TAYLOR_DEFS[0]: taylor[TAYLOR_DEFS[0]],
                         TAYLOR_DEFS[1]: from_taylor_terms})
    dirty_list, psf_list = _image_list(dirty), _image_list(psf)
    window_list = ns["find_window_list"](dirty_list, "", window_shape="quarter")
    comp_list, residual_list = ns["mmclean_kernel_list"](dirty_list, "", psf_list, window_list,
                                                         None, **kwargs)
    comp = np.concatenate([im["pixels"].data for im in comp_list])
    residual = np.concatenate([im["pixels"].data for im in residual_list])
    if not (comp[:, 0].any() and comp[:, 1].any()):
        raise Rejected("L1 left a polarisation without components")
    moments_of = taylor["calculate_image_list_frequency_moments"]
    dirty_moments = moments_of(dirty_list, nmoment=2)["pixels"].data
    psf_moments = moments_of(psf_list, nmoment=4)["pixels"].data
    print(f"L1: cycles per polarisation {counts}, min gap {min(gaps):.2e}")
    inputs = dict(dirty=dirty, psf=psf, f0=F0, bw=BW)
    outputs = dict(comp=comp, residual=residual, dirty_moments=dirty_moments,
                   psf_moments=psf_moments, comp_moments=cleaned_moments[0],
                   residual_moments=cleaned_moments[1], min_gap=min(gaps), window_shape="quarter",
                   **{k: (np.array(v, dtype=float) if k == "scales" else v) for k, v in kwargs.items()})
    return inputs, outputs


def make_mfsclean():
    for seed in range(5, 60):
        try:
            inp = make_inputs(seed)
            cases = make_cases(inp)
            list_in, list_out = make_list_case(seed)
        except Rejected as e:
            print(f"seed {seed}: {e.args[0]}, trying the next")
            continue
        save("mfsclean_inputs.npz", seed=seed, **inp)
        for name, arrays in cases.items():
            save(f"mfsclean_{name}.npz", seed=seed, **arrays)
        save("mfsclean_L1_inputs.npz", seed=seed, **list_in)
        save("mfsclean_L1.npz", seed=seed, **list_out)
        return
    raise RuntimeError("no seed met the conditions")


if __name__ == "__main__":
    make_mfsclean()
