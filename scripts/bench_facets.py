"""Time the gather of overlapping image facets (csrc/facets.hip through
image/gather_scatter.py) on one GPU.

Workload: one 1 x stokesIQUV x 8192 x 8192 float64 image (2.1 GB) gathered
from 8 x 8 facets of 1024 x 1024 pixels that overlap by 32 pixels, with the
linear taper; every facet is a tensor of its own, as a faceted deconvolution
leaves them.

Timed, alternating, with device events around the call, after warm-up calls:
  fused   image_gather_facets on device pixels: one kernel call
  kernel  kernels.gather_facets alone on the same facets (its time gives the
          achieved bandwidth)
  loop    the reference's gather transcribed to torch operations on the device
          (copied below as the baseline): F^2 taper images, per facet a
          multiply into a temporary and two read-modify-writes of image
          windows, then the masked division

Bytes: the kernel reads every facet pixel once and writes every image pixel
once.  The loop, counted in facet-sized and image-sized passes: per facet 1
write for its flat, 3 for the multiply, 3 + 3 for the two additions into
windows (10 facet passes); 3 image writes for the zeroed / filled images and
about 9 image passes for the two masks, the masked division (gather of both
operands, scatter of the quotient) and the masked zeroing.  The outputs of
the two paths are compared bit for bit.  Prints one JSON line;
"fused_slowest_below_loop_fastest" is the acceptance check.

  python scripts/bench_facets.py [--npix 8192] [--facets 8] [--overlap 32] [--repeats 7]
"""

import argparse
import json
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-python_amd"))

from ska_sdp_func_python_amd import datamodels as dm  # noqa: E402
from ska_sdp_func_python_amd import kernels  # noqa: E402
from ska_sdp_func_python_amd.image import gather_scatter, iterators  # noqa: E402


# ---- the baseline: the reference's image_gather_facets in torch operations ----
def loop_gather(image_list, im, facets, overlap, taper):
    pixels = im["pixels"].data

    def like(fill):
        return dm.Image.constructor(torch.full_like(pixels, fill), im.image_acc.polarisation_frame,
                                    im.image_acc.wcs)

    out, sum_flats = like(0.0), like(0.0)
    flats = list(iterators.image_raster_iter(like(1.0), facets=facets, overlap=overlap, taper=taper,
                                             make_flat=True))
    for i, (out_facet, sum_flat_facet) in enumerate(zip(
            iterators.image_raster_iter(out, facets=facets, overlap=overlap, taper=taper),
            iterators.image_raster_iter(sum_flats, facets=facets, overlap=overlap, taper=taper))):
        out_facet["pixels"].data[...] += flats[i]["pixels"].data * image_list[i]["pixels"].data[...]
        sum_flat_facet["pixels"].data[...] += flats[i]["pixels"].data[...]
    out["pixels"].data[sum_flats["pixels"].data > 0.0] /= \
        sum_flats["pixels"].data[sum_flats["pixels"].data > 0.0]
    out["pixels"].data[sum_flats["pixels"].data <= 0.0] = 0.0
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def measure(variants, warmup, repeats):
    """{name: [ms per repeat]} of the variants, alternating between them."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    times = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            times[name].append(timed(fn)[0])
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=8192)
    ap.add_argument("--facets", type=int, default=8)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--taper", default="linear")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_facets.py needs a GPU: it measures nothing on the host")
    dev = torch.device("cuda:0")
    n, facets, overlap, npol = args.npix, args.facets, args.overlap, 4
    pf = dm.PolarisationFrame("stokesIQUV")
    im = dm.create_image(8, 1e-4, dm.SkyCoord(0.2, -0.7), polarisation_frame=pf)
    gen = torch.Generator(device=dev).manual_seed(0)
    im["pixels"].data = torch.randn((1, npol, n, n), dtype=torch.float64, device=dev, generator=gen)
    image_list = [dm.Image.constructor(v["pixels"].data.clone(), pf, v.image_acc.wcs)
                  for v in gather_scatter.image_scatter_facets(im, facets=facets, overlap=overlap)]
    dy, dx, sy, sx, y0, x0 = iterators.raster_geometry(im, facets, overlap)
    planes = [v["pixels"].data for v in image_list]
    taper_y = iterators.taper_1d(args.taper, dy, overlap)
    taper_x = iterators.taper_1d(args.taper, dx, overlap)

    times = measure({
        "fused": lambda: gather_scatter.image_gather_facets(image_list, im, facets, overlap,
                                                            args.taper),
        "loop": lambda: loop_gather(image_list, im, facets, overlap, args.taper),
        "kernel": lambda: kernels.gather_facets(planes, facets, (n, n), (y0, x0), (sy, sx), taper_y,
                                                taper_x, normalise=True)},
        args.warmup, args.repeats)
    a = gather_scatter.image_gather_facets(image_list, im, facets, overlap, args.taper)
    b = loop_gather(image_list, im, facets, overlap, args.taper)
    equal = bool(torch.equal(a["pixels"].data.view(torch.int64), b["pixels"].data.view(torch.int64)))

    image_bytes = npol * n * n * 8
    facet_bytes = facets * facets * npol * dy * dx * 8
    moved = facet_bytes + image_bytes
    loop_moved = 10 * facet_bytes + 12 * image_bytes
    fused, loop, kernel = times["fused"], times["loop"], times["kernel"]
    med = lambda v: float(numpy.median(v))
    print(json.dumps({
        "step": "gather_facets", "npix": n, "npol": npol, "dtype": "float64", "facets": facets,
        "overlap": overlap, "taper": args.taper, "facet_pixels": [dy, dx],
        "fused_ms_median": med(fused), "fused_ms_min": min(fused), "fused_ms_max": max(fused),
        "kernel_ms_median": med(kernel), "kernel_ms_min": min(kernel), "kernel_ms_max": max(kernel),
        "loop_ms_median": med(loop), "loop_ms_min": min(loop), "loop_ms_max": max(loop),
        "fused_slowest_below_loop_fastest": max(fused) < min(loop),
        "speedup_median": med(loop) / med(fused),
        "bytes_moved": moved, "loop_bytes_moved_model": loop_moved,
        "traffic_model_ratio": loop_moved / moved,
        "kernel_tb_per_s_median": moved / (1e-3 * med(kernel)) / 1e12,
        "kernel_tb_per_s_range": [moved / (1e-3 * max(kernel)) / 1e12,
                                  moved / (1e-3 * min(kernel)) / 1e12],
        "loop_tb_per_s_model": loop_moved / (1e-3 * med(loop)) / 1e12,
        "bit_equal_to_loop": equal}), flush=True)


if __name__ == "__main__":
    main()
