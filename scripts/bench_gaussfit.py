"""Time the batched Gaussian fit (csrc/gaussfit.hip) and
find_skycomponents_frequency_taylor_terms on one GPU.

Workload: 16 single-channel stokesI float64 images of 2048 x 2048 that hold
1,000 components restored with a circular beam of sigma 1.5 pixels, their
fluxes following a spectral index, on noise of 0.01: 16,000 fits of 15 x 15
pixels.

Measured with device events, after warm-up calls, median of the repeats:
  * kernels.gauss_fit alone on the 16,000 windows (the library call: the copy of
    its tables and the kernel), with the iterations it took;
  * the whole find_skycomponents_frequency_taylor_terms call (moment 0, the
    find, the fits, the flux gathers and the host steps), also by a host clock
    around a device synchronise;
  * the host path the fit replaces: the copy of plane [0, 0] of every image to
    the host, once, and the scipy restatement (tests/gaussfit_restatement.py,
    MINPACK through scipy.optimize.leastsq at the reference's stop) on a sample
    of the fits, extrapolated to all of them.  The sample size is printed.
The device's parameters are compared with the restatement's on the sample.
Prints JSON lines.

  python scripts/bench_gaussfit.py [--npix 2048] [--nchan 16] [--ncomp 1000] [--sample 400]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gaussfit_restatement as G  # noqa: E402
import skycomp_restatement as R  # noqa: E402
from ska_sdp_func_python_amd import kernels  # noqa: E402
from ska_sdp_func_python_amd.image.deconvolution import _gaussian_coefficients  # noqa: E402
from ska_sdp_func_python_amd.sky_component import taylor_terms as tt  # noqa: E402


def event_ms(fn, warmup, repeats):
    """Median device-event and host-clock milliseconds of fn(), and its last result."""
    for _ in range(warmup):
        out = fn()
    dev_ms, host_ms = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(e0.elapsed_time(e1))
    return float(np.median(dev_ms)), float(np.median(host_ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=2048)
    ap.add_argument("--nchan", type=int, default=16)
    ap.add_argument("--ncomp", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=400, help="fits of the host path that are run")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gaussfit.py needs a GPU: it measures nothing on the host alone")
    dev = torch.device("cuda:0")
    n, nchan, ncomp = args.npix, args.nchan, args.ncomp

    # components on a jittered lattice, so that no two fitting windows overlap
    rng = np.random.default_rng(0)
    side = int(np.ceil(np.sqrt(ncomp)))
    pitch = n / side
    if pitch < 40:
        raise SystemExit("too many components for the image: their windows would overlap")
    cells = rng.permutation(side * side)[:ncomp]
    xy = np.stack([(cells % side + 0.5) * pitch, (cells // side + 0.5) * pitch], axis=1)
    xy += rng.uniform(-0.25 * pitch + 8, 0.25 * pitch - 8, xy.shape)
    freqs = 1.0e9 * (1.0 + 0.02 * np.arange(nchan))
    flux0 = rng.uniform(1.0, 10.0, ncomp)
    alpha = rng.uniform(-1.2, 0.2, ncomp)
    torch.manual_seed(0)
    images = []
    for chan, f in enumerate(freqs):
        pixels = 0.01 * torch.randn((1, 1, n, n), dtype=torch.float64, device=dev)
        flux = (flux0 * (f / freqs[nchan // 2]) ** alpha)[:, None, None]
        kernels.skycomp_restore(pixels, xy, flux, *_gaussian_coefficients(1.5, 1.5, 0.0))
        g = R.geometry(1, "stokesI")
        g.update(shape=np.array([n, n]), cell_deg=2.0 / n, frequency=f, channel_bandwidth=0.02e9)
        images.append(R.make_image(g, pixels=pixels, to=lambda p: p))

    # ---- the kernel alone ----
    planes = [plane for im in images for plane in [im["pixels"].data[0, 0]] * ncomp]
    x0 = np.tile(np.round(xy[:, 0]).astype(np.int64) - G.HALF, nchan)
    y0 = np.tile(np.round(xy[:, 1]).astype(np.int64) - G.HALF, nchan)
    dev_ms, host_ms, (params, status, niter) = event_ms(
        lambda: kernels.gauss_fit(planes, x0, y0), args.warmup, args.repeats)
    it = niter.cpu().numpy()
    print(json.dumps({"op": "gauss_fit", "nfit": len(planes), "npix": n, "device_ms": dev_ms,
                      "host_clock_ms": host_ms, "us_per_fit": 1e3 * dev_ms / len(planes),
                      "status_counts": np.bincount(status.cpu().numpy(), minlength=3).tolist(),
                      "evaluations_min_median_max": [int(it.min()), float(np.median(it)),
                                                     int(it.max())]}), flush=True)

    # ---- the whole call ----
    find = lambda: tt.find_skycomponents_frequency_taylor_terms(images, nmoment=3,
                                                                component_threshold=0.5)
    dev_ms, host_ms, found = event_ms(find, 1, args.repeats)
    whole = {"op": "find_skycomponents_frequency_taylor_terms", "nchan": nchan, "npix": n,
             "nmoment": 3, "components_found": len(found[0]) if found else 0,
             "device_event_ms": dev_ms, "host_clock_ms": host_ms}
    print(json.dumps(whole), flush=True)

    # ---- the host path: copy plane [0, 0] of every image, one scipy fit per window ----
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_planes = [im["pixels"].data[0, 0].cpu().numpy() for im in images]
    copy_ms = 1e3 * (time.perf_counter() - t0)
    sample = rng.permutation(len(planes))[:args.sample]
    p_dev = params.cpu().numpy()
    worst = np.zeros(6)
    t0 = time.perf_counter()
    nfev = []
    for f in sample:
        fit = G.fit_plane(host_planes[f // ncomp], int(x0[f]), int(y0[f]))
        nfev.append(fit["nfev"])
        d = np.abs(fit["params"] - p_dev[f])
        d[5] = 0.0   # circular sources: theta is not determined
        worst = np.maximum(worst, d)
    fit_ms = 1e3 * (time.perf_counter() - t0)
    total = copy_ms + fit_ms * len(planes) / len(sample)
    print(json.dumps({"op": "host_path", "copy_ms": copy_ms, "sample": len(sample),
                      "sample_fit_ms": fit_ms, "ms_per_fit": fit_ms / len(sample),
                      "evaluations_median": float(np.median(nfev)),
                      "extrapolated_total_ms": total,
                      "extrapolated_over_whole_call": total / whole["host_clock_ms"],
                      "max_abs_difference_device_vs_reference_stop": worst[:5].tolist()}),
          flush=True)


if __name__ == "__main__":
    main()
