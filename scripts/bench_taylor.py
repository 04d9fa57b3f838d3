"""Time the frequency-moment steps of multi-frequency synthesis (csrc/taylor.hip
through image/taylor_terms.py) on one GPU.

Workload: a list of 16 single-channel 2048 x 2048 stokesIQUV float64 images
(2.1 GB), each a tensor of its own as deconvolve_list holds them:
  moments  calculate_image_list_frequency_moments, 6 moments (the PSF moments
           of a 3-moment clean): 16 planes in, 6 out
  rebuild  calculate_image_list_from_frequency_taylor_terms, the 16 channels
           from 3 Taylor terms: 3 planes in, 16 out

Each step is timed as the fused kernel path and as the torch-op loop that the
functions ran before the kernel existed (copied below as the baseline: per
moment and channel a full-image multiply into a temporary and a full-image
add), alternating, with device events around the call, after warm-up calls.
The fused kernel alone (kernels.mix_planes on the same planes) is timed too;
its time gives the achieved bandwidth.  Bytes: the fused pass reads every
input plane once and writes every output plane once; a loop round moves five
planes (multiply: one read, one write; add: two reads, one write).  The
outputs of the two paths are compared bit for bit.  Prints one JSON line per
step; "fused_slowest_below_loop_fastest" is the acceptance check.

  python scripts/bench_taylor.py [--npix 2048] [--nchan 16] [--nmoment 3] [--repeats 7]
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
from ska_sdp_func_python_amd.image import taylor_terms as tt  # noqa: E402


# ---- the baseline: the torch-op loops of the two list functions before the kernel ----
def loop_moments(im_list, nmoment):
    nchan = len(im_list)
    first = im_list[0]["pixels"].data
    _, npol, ny, nx = first.shape
    freq = tt._channel_frequencies(im_list)
    reference_frequency = freq[nchan // 2]
    moment_data = torch.zeros((nmoment, npol, ny, nx), dtype=torch.float64, device=first.device)
    for moment in range(nmoment):
        for chan, im in enumerate(im_list):
            weight = numpy.power((freq[chan] - reference_frequency) / reference_frequency, moment)
            moment_data[moment] += im["pixels"].data[0] * float(weight[0])
    return moment_data


def loop_rebuild(im_list, moments):
    nchan, nmoment = len(im_list), moments.shape[0]
    frequency = numpy.array([d.frequency.data[0] for d in im_list])
    reference_frequency = frequency[nchan // 2]
    out = []
    for chan in range(nchan):
        newim_data = torch.zeros(tuple(im_list[chan]["pixels"].data.shape), dtype=torch.float64,
                                 device=moments.device)
        for moment in range(nmoment):
            weight = numpy.power((frequency[chan] - reference_frequency) / reference_frequency,
                                 moment)
            newim_data[0] += moments[moment] * float(weight)
        out.append(newim_data)
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


def report(step, times, nin, nout, nrounds, plane_bytes, equal, shape):
    fused, loop, kernel = times["fused"], times["loop"], times["kernel"]
    moved = (nin + nout) * plane_bytes
    loop_moved = 5 * nrounds * plane_bytes
    med = lambda v: float(numpy.median(v))
    print(json.dumps({
        "step": step, **shape, "planes_in": nin, "planes_out": nout,
        "fused_ms_median": med(fused), "fused_ms_max": max(fused),
        "loop_ms_median": med(loop), "loop_ms_min": min(loop),
        "kernel_ms_median": med(kernel),
        "fused_slowest_below_loop_fastest": max(fused) < min(loop),
        "speedup_median": med(loop) / med(fused),
        "bytes_moved": moved, "loop_bytes_moved_model": loop_moved,
        "traffic_model_ratio": loop_moved / moved,
        "kernel_tb_per_s": moved / (1e-3 * med(kernel)) / 1e12,
        "loop_tb_per_s_model": loop_moved / (1e-3 * med(loop)) / 1e12,
        "bit_equal_to_loop": equal}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=2048)
    ap.add_argument("--nchan", type=int, default=16)
    ap.add_argument("--nmoment", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_taylor.py needs a GPU: it measures nothing on the host")
    dev = torch.device("cuda:0")
    n, nchan, nmoment, npol = args.npix, args.nchan, args.nmoment, 4
    pf = dm.PolarisationFrame("stokesIQUV")
    gen = torch.Generator(device=dev).manual_seed(0)
    im_list = []
    for chan in range(nchan):
        im = dm.create_image(8, 1e-4, dm.SkyCoord(0.2, -0.7), polarisation_frame=pf,
                             frequency=1.0e8 + 3.0e6 * chan, channel_bandwidth=3.0e6)
        im["pixels"].data = torch.randn((1, npol, n, n), dtype=torch.float64, device=dev,
                                        generator=gen)
        im_list.append(im)
    plane_bytes = npol * n * n * 8
    shape = {"npix": n, "nchan": nchan, "npol": npol, "dtype": "float64"}
    planes = [im["pixels"].data[0] for im in im_list]

    # ---- moments: nchan planes -> 2 nmoment planes ----
    npsf = 2 * nmoment
    w = numpy.random.default_rng(0).normal(size=(npsf, nchan))
    out = torch.empty((npsf, npol, n, n), dtype=torch.float64, device=dev)
    times = measure({
        "fused": lambda: tt.calculate_image_list_frequency_moments(im_list, nmoment=npsf),
        "loop": lambda: loop_moments(im_list, npsf),
        "kernel": lambda: kernels.mix_planes(planes, w, out)}, args.warmup, args.repeats)
    del out
    fused = tt.calculate_image_list_frequency_moments(im_list, nmoment=npsf)["pixels"].data
    equal = bool(torch.equal(fused.view(torch.int64), loop_moments(im_list, npsf).view(torch.int64)))
    report("moments", times, nchan, npsf, npsf * nchan, plane_bytes, equal, shape)

    # ---- rebuild: nmoment planes -> nchan planes ----
    moment_image = dm.Image.constructor(fused[:nmoment].clone(), pf, im_list[0].image_acc.wcs)
    del fused
    terms = list(moment_image["pixels"].data)
    w = numpy.random.default_rng(1).normal(size=(nchan, nmoment))
    out = torch.empty((nchan, npol, n, n), dtype=torch.float64, device=dev)
    times = measure({
        "fused": lambda: tt.calculate_image_list_from_frequency_taylor_terms(im_list, moment_image),
        "loop": lambda: loop_rebuild(im_list, moment_image["pixels"].data),
        "kernel": lambda: kernels.mix_planes(terms, w, out)}, args.warmup, args.repeats)
    del out
    a = tt.calculate_image_list_from_frequency_taylor_terms(im_list, moment_image)
    b = loop_rebuild(im_list, moment_image["pixels"].data)
    equal = all(torch.equal(x["pixels"].data.contiguous().view(torch.int64), y.view(torch.int64))
                for x, y in zip(a, b))
    report("rebuild", times, nmoment, nchan, nmoment * nchan, plane_bytes, equal, shape)


if __name__ == "__main__":
    main()
