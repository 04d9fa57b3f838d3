"""Time find_skycomponents (csrc/segment.hip) on one GPU.

Workload: a 4096 x 4096 stokesIQUV float64 cube of 8 channels (4.3 GB) that
holds 1,000 components restored with a beam of 3.5 pixels FWHM on noise of
0.05; find_skycomponents(fwhm, threshold=0.5, npixels=5) with fwhm 1 (no
smoothing) and, with --fwhm, a smoothed run.

Measured, after warm-up calls, median of the repeats:
  * every library call of the find with device events around it (label = mean
    + smooth + threshold + tile labels, border merge, flatten; roots; relabel;
    peaks), and the whole find_skycomponents call with a host clock around a
    device synchronise;
  * the host path it replaces, once: the device -> host copy of the cube, then
    the restatement's steps from numpy and scipy.ndimage.label (the peaks
    through each segment's bounding box);
  * kernels.mix_planes on the same 8 Stokes-I planes (8 read, 1 written), which
    puts the streaming stages in terms of bytes per second.
The segment maps of the two paths are compared.  Prints JSON lines.  The
kernels of the label call are told apart by a kernel trace of this script
(--repeats 1), not here.

  python scripts/bench_findcomp.py [--npix 4096] [--nchan 8] [--ncomp 1000] [--fwhm 3]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import findcomp_restatement as F  # noqa: E402
import skycomp_restatement as R  # noqa: E402
from ska_sdp_func_python_amd import _lib, kernels  # noqa: E402
from ska_sdp_func_python_amd.image.deconvolution import _gaussian_coefficients  # noqa: E402
from ska_sdp_func_python_amd.sky_component import operations as ops  # noqa: E402


class CallTimer:
    """Device events around every launch that goes through _lib.call, by name."""

    def __init__(self):
        self.real = _lib.call
        self.events = []

    def __enter__(self):
        def timed(name, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.real(name, *args)
            e1.record()
            self.events.append((name, e0, e1))
        _lib.call = timed
        return self

    def __exit__(self, *exc):
        _lib.call = self.real

    def ms(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.events:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        self.events = []
        return out


def host_path(cube_dev, kernel, threshold, npixels):
    """Copy the cube to the host and run the restatement's steps 1-4 there."""
    t = {}
    t0 = time.perf_counter()
    cube = cube_dev.cpu().numpy()
    t["copy_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    planes = cube[:, 0]
    smoothed = F.smooth(F.mean_plane(planes), kernel)
    t["mean_smooth_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    labels, n = F.label_mask(smoothed > threshold, npixels)
    t["label_ms"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    nx = labels.shape[1]
    values = np.zeros((planes.shape[0], n))
    indices = np.zeros((planes.shape[0], n), dtype=np.int64)
    for seg, box in enumerate(ndimage.find_objects(labels)):
        inside = labels[box] == seg + 1
        rows, cols = np.nonzero(inside)
        for chan in range(planes.shape[0]):
            v = planes[chan][box][inside]
            first = int(np.argmax(v))
            values[chan, seg] = v[first]
            indices[chan, seg] = (box[0].start + rows[first]) * nx + box[1].start + cols[first]
    t["peaks_ms"] = 1e3 * (time.perf_counter() - t0)
    t["total_ms"] = sum(t.values())
    return labels, n, values, indices, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=4096)
    ap.add_argument("--nchan", type=int, default=8)
    ap.add_argument("--ncomp", type=int, default=1000)
    ap.add_argument("--fwhm", type=float, default=3.0, help="the smoothed run (0: none)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_findcomp.py needs a GPU: it measures nothing on the host")
    dev = torch.device("cuda:0")
    n, nchan, npol = args.npix, args.nchan, 4
    rng = np.random.default_rng(0)
    xy = rng.uniform(8.0, n - 9.0, (args.ncomp, 2))
    flux = np.zeros((args.ncomp, nchan, npol))
    flux[:, :, 0] = rng.uniform(1.0, 10.0, (args.ncomp, 1)) * rng.uniform(0.8, 1.25, (args.ncomp, nchan))
    flux[:, :, 1:] = 0.1 * flux[:, :, :1]
    torch.manual_seed(0)
    cube = 0.05 * torch.randn((nchan, npol, n, n), dtype=torch.float64, device=dev)
    sigma = 3.5 / np.sqrt(8.0 * np.log(2.0))
    kernels.skycomp_restore(cube, xy, flux, *_gaussian_coefficients(sigma, sigma, 0.0))
    g = R.geometry(nchan, "stokesIQUV")
    g["shape"] = np.array([n, n])
    g["cell_deg"] = 2.0 / n
    im = R.make_image(g, pixels=cube, to=lambda p: p)
    threshold, npixels = 0.5, 5
    plane_bytes = n * n * 8

    # ---- mix_planes on the same planes: the streaming yardstick ----
    ins = [cube[c, 0] for c in range(nchan)]
    out = torch.empty((1, n, n), dtype=torch.float64, device=dev)
    w = np.full((1, nchan), 1.0 / nchan)
    for _ in range(args.warmup):
        kernels.mix_planes(ins, w, out)
    ms = []
    with CallTimer() as ct:
        for _ in range(args.repeats):
            kernels.mix_planes(ins, w, out)
            ms.append(sum(ct.ms().values()))
    mix_ms = float(np.median(ms))
    mix_bytes = (nchan + 1) * plane_bytes
    print(json.dumps({"op": "mix_planes", "npix": n, "nin": nchan, "nout": 1, "kernel_ms": mix_ms,
                      "bytes": mix_bytes, "TB_per_s": mix_bytes / mix_ms * 1e-9}), flush=True)

    for fwhm in [1.0] + ([args.fwhm] if args.fwhm > 1.0 else []):
        find = lambda: ops.find_skycomponents(im, fwhm=fwhm, threshold=threshold, npixels=npixels)
        for _ in range(args.warmup):
            comps = find()
        torch.cuda.synchronize()
        calls, whole = [], []
        with CallTimer() as ct:
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                comps = find()
                torch.cuda.synchronize()
                whole.append(1e3 * (time.perf_counter() - t0))
                calls.append(ct.ms())
        med = {k.replace("sdp_hip_", "") + "_ms": float(np.median([c[k] for c in calls]))
               for k in calls[0]}
        border = ((n - 1) // _lib.SDP_HIP_SEGMENT_TILE) * 2 * n
        rec = {"op": "find_skycomponents", "npix": n, "nchan": nchan, "npol": npol, "fwhm": fwhm,
               "kernel_size": ops.segment_kernel(fwhm).shape[0], "components_found": len(comps),
               **med, "library_calls_ms": float(sum(med.values())),
               "whole_call_ms": float(np.median(whole)),
               "whole_call_ms_range": [float(min(whole)), float(max(whole))],
               "label_bytes_min": (nchan + 1) * plane_bytes,
               "label_as_multiple_of_mix_planes": med["segment_label_ms"] / mix_ms,
               "border_pixels_per_pixel": border / float(n * n)}
        labels, nlab = ops.segment_image(im, fwhm=fwhm, threshold=threshold, npixels=npixels)
        rec["foreground_fraction"] = float((labels > 0).double().mean())
        if not args.no_host:
            hl, hn, hv, hi, t = host_path(cube, ops.segment_kernel(fwhm), threshold, npixels)
            v, i = kernels.segment_peaks(cube[:, 0], labels, nlab)
            rec["host_path"] = t
            rec["labels_equal_to_host"] = bool(hn == nlab and np.array_equal(labels.cpu().numpy(), hl))
            rec["peaks_equal_to_host"] = bool(np.array_equal(v.cpu().numpy(), hv)
                                              and np.array_equal(i.cpu().numpy(), hi))
            rec["host_over_device"] = t["total_ms"] / rec["whole_call_ms"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
