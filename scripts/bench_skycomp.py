"""Time the sky-component image kernels (csrc/skycomp.hip) on one GPU.

Workload: a 4096 x 4096 stokesIQUV float64 image (one channel, 0.5 GB) and
10,000 point components at random positions:
  insert   Lanczos, support 8 (windows of 16 x 16 pixels)
  restore  a circular clean beam of 3.5 pixels FWHM
  nearest  the Voronoi label image of the first 1,000 components

Each kernel is timed with device events around its launch, after warm-up
calls, median of the repeats; the whole wrapper call (per-tile lists made on
the host, uploads, kernel) is timed with a host clock around a device
synchronise.  Beside each stands the time of the sequential numpy restatement
(tests/skycomp_restatement.py) on the same inputs: insert in full; restore
EXTRAPOLATED from its first 20 components (each is a full-image Gaussian);
nearest EXTRAPOLATED from the first 8 image rows.  Bytes: what each kernel
reads and writes of the image (tiles with a non-empty list, read and written
once; the label image written once) against one read plus one write of the
whole image.  Prints one JSON line per operation.

  python scripts/bench_skycomp.py [--npix 4096] [--ncomp 10000] [--repeats 5]
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

import skycomp_restatement as R  # noqa: E402
from ska_sdp_func_python_amd import _lib, kernels  # noqa: E402
from ska_sdp_func_python_amd.image.deconvolution import _gaussian_coefficients  # noqa: E402
from ska_sdp_func_python_amd.sky_component.operations import insert_function_L, insert_taps  # noqa: E402


class KernelTimer:
    """Device events around every launch that goes through _lib.call."""

    def __init__(self):
        self.real = _lib.call
        self.events = []

    def __enter__(self):
        def timed(name, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.real(name, *args)
            e1.record()
            self.events.append((e0, e1))
        _lib.call = timed
        return self

    def __exit__(self, *exc):
        _lib.call = self.real

    def ms(self):
        torch.cuda.synchronize()
        total = sum(e0.elapsed_time(e1) for e0, e1 in self.events)
        self.events = []
        return total


def measure(fn, warmup, repeats):
    """(median kernel ms, median wrapper ms) of fn()."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    kernel, whole = [], []
    with KernelTimer() as kt:
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            whole.append(1e3 * (time.perf_counter() - t0))
            kernel.append(kt.ms())
    return float(np.median(kernel)), float(np.median(whole))


def tile_traffic(boxes, ncomp, ny, nx, nplanes):
    """Image bytes read plus written by a tiled kernel, and its (tile, component) pairs."""
    ptr, comp = kernels.tile_csr(boxes, 0, ncomp, ny, nx, torch.device("cuda:0"))
    tiles = int(torch.count_nonzero(torch.diff(ptr)))
    pixels = tiles * _lib.SDP_HIP_SKYCOMP_TILE_X * _lib.SDP_HIP_SKYCOMP_TILE_Y
    return 2 * 8 * nplanes * pixels, int(comp.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=4096)
    ap.add_argument("--ncomp", type=int, default=10000)
    ap.add_argument("--nvoronoi", type=int, default=1000)
    ap.add_argument("--fwhm", type=float, default=3.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skycomp.py needs a GPU: it measures nothing on the host")
    dev = torch.device("cuda:0")
    n, ncomp, npol, S = args.npix, args.ncomp, 4, 8
    rng = np.random.default_rng(0)
    xy = rng.uniform(S + 1.0, n - S - 1.0, (ncomp, 2))
    flux = rng.uniform(0.1, 10.0, (ncomp, 1, npol))
    image = torch.zeros((1, npol, n, n), dtype=torch.float64, device=dev)
    image_bytes = 2 * image.numel() * 8

    # ---- insert ----
    t0 = time.perf_counter()
    taps = [insert_taps(x, y, 1.0, S, insert_function_L) for x, y in xy]
    host_ms = 1e3 * (time.perf_counter() - t0)
    origin = np.array([t[0] for t in taps])
    ty, tx = np.array([t[1] for t in taps]), np.array([t[2] for t in taps])
    isum = np.array([t[3] for t in taps])
    k_ms, w_ms = measure(lambda: kernels.skycomp_insert(image, origin, ty, tx, isum, flux),
                         args.warmup, args.repeats)
    host = np.zeros((1, npol, n, n))
    t0 = time.perf_counter()
    R.insert(host, origin, ty, tx, isum, flux)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    image.zero_()
    kernels.skycomp_insert(image, origin, ty, tx, isum, flux)
    equal = bool(np.array_equal(image.cpu().numpy(), host))
    boxes = kernels.tile_boxes(origin[:, 0], origin[:, 0] + 2 * S - 1, origin[:, 1],
                                origin[:, 1] + 2 * S - 1, n, n)
    moved, pairs = tile_traffic(boxes, ncomp, n, n, npol)
    print(json.dumps({"op": "insert", "npix": n, "ncomp": ncomp, "method": "Lanczos", "support": S,
                      "kernel_ms": k_ms, "wrapper_ms": w_ms, "host_taps_ms": host_ms,
                      "numpy_ms": numpy_ms, "bit_equal_to_numpy": equal, "tile_pairs": pairs,
                      "image_bytes_moved": moved, "image_read_plus_write_bytes": image_bytes}))
    del host

    # ---- restore ----
    sigma = args.fwhm / np.sqrt(8.0 * np.log(2.0))
    a, b, c = _gaussian_coefficients(sigma, sigma, 0.0)
    image.zero_()
    k_ms, w_ms = measure(lambda: kernels.skycomp_restore(image, xy, flux, a, b, c),
                         args.warmup, args.repeats)
    nref = min(20, ncomp)
    image.zero_()
    kernels.skycomp_restore(image, xy[:nref], flux[:nref], a, b, c)
    host = np.zeros((1, npol, n, n))
    t0 = time.perf_counter()
    R.restore(host, xy[:nref], flux[:nref], a, b, c)
    numpy_ms = 1e3 * (time.perf_counter() - t0) * ncomp / nref
    err = float(np.abs(image.cpu().numpy() - host).max() / np.abs(flux[:nref]).sum(axis=0).max())
    r = np.sqrt(kernels.RESTORE_SKIP_ARGUMENT / (a * (1.0 - 1e-9))) + 1.0
    boxes = kernels.tile_boxes(np.floor(xy[:, 0] - r), np.ceil(xy[:, 0] + r),
                                np.floor(xy[:, 1] - r), np.ceil(xy[:, 1] + r), n, n)
    moved, pairs = tile_traffic(boxes, ncomp, n, n, npol)
    print(json.dumps({"op": "restore", "npix": n, "ncomp": ncomp, "fwhm_pixels": args.fwhm,
                      "kernel_ms": k_ms, "wrapper_ms": w_ms,
                      "numpy_ms_extrapolated_from_20_components": numpy_ms,
                      "max_error_over_sum_flux_20_components": err, "tile_pairs": pairs,
                      "pixel_component_pairs": pairs * 256, "image_bytes_moved": moved,
                      "image_read_plus_write_bytes": image_bytes}))
    del host

    # ---- nearest ----
    nv = min(args.nvoronoi, ncomp)
    pts = xy[:nv]
    k_ms, w_ms = measure(lambda: kernels.skycomp_nearest(n, n, pts, dev), args.warmup, args.repeats)
    labels = kernels.skycomp_nearest(n, n, pts, dev).cpu().numpy()
    rows = 8
    t0 = time.perf_counter()
    ref = R.nearest(rows, n, pts)
    numpy_ms = 1e3 * (time.perf_counter() - t0) * n / rows
    print(json.dumps({"op": "nearest", "npix": n, "ncomp": nv, "kernel_ms": k_ms, "wrapper_ms": w_ms,
                      "numpy_ms_extrapolated_from_8_rows": numpy_ms,
                      "equal_to_numpy_on_8_rows": bool(np.array_equal(labels[:rows], ref)),
                      "label_bytes_written": n * n * 8,
                      "image_read_plus_write_bytes": image_bytes}))


if __name__ == "__main__":
    main()
