"""Time the glue between imaging calls (csrc/imgsum.hip through
imaging/imaging_helpers.py) on one GPU.

Three steps, each against its transcription as torch operations and, for the
two image steps, against kernels.mix_planes moving the same bytes in the same
session (both kernels have its access pattern, so its bandwidth is the
yardstick):

  sum_invert   sum_invert_results on 16 results of 4096 x 4096 stokesIQUV
               float64: kernels.sum_planes alone, the whole call, the torch
               loop (acc += w * x per entry, then the divide), and mix_planes
               with 16 planes in and 1 out of the same size
  threshold    threshold_list on a 16-channel 2048 x 2048 stokesIQUV float64
               cube and on its 8 x 8 facet views with overlap 32:
               kernels.peak_abs alone, the whole call on the cube and on the
               64 views, calculate_image_frequency_moments + abs + amax, and
               mix_planes with the 16 channels in and 1 plane out
  sum_predict  sum_predict_results on 4 Visibilities of 100 x 19306 x 64 x 4
               complex64 against the torch `+=` loop

The variants of a step alternate; every call is timed with device events
after warm-up calls.  Medians with min and max go to one JSON line per step;
"bytes" is what a variant must move (every input read once, every output
written once) and "tb_per_s" follows from the median.  Everything is seeded.

  python scripts/bench_imaging_helpers.py [--repeats 11] [--warmup 2] [--scale 1.0]

``--scale`` below 1 shrinks every image side and the visibility rows.
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
from ska_sdp_func_python_amd.image.gather_scatter import image_scatter_facets  # noqa: E402
from ska_sdp_func_python_amd.image.taylor_terms import calculate_image_frequency_moments  # noqa: E402
from ska_sdp_func_python_amd.imaging import imaging_helpers as ih  # noqa: E402

PF = dm.PolarisationFrame("stokesIQUV")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(variants, warmup, repeats):
    """{name: [ms per repeat]} of the variants, alternating between them."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    times = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    return times


def report(step, shape, times, moved, checks):
    out = {"step": step, **shape}
    for name, ms in times.items():
        med = float(numpy.median(ms))
        out[name] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "n": len(ms)}
        if name in moved:
            out[name]["bytes"] = moved[name]
            out[name]["tb_per_s"] = moved[name] / (1e-3 * med) / 1e12
    out.update(checks)
    print(json.dumps(out), flush=True)


def image(pixels, f0=1.0e8):
    im = dm.create_image(8, 1e-4, dm.SkyCoord(0.2, -0.7), polarisation_frame=PF, frequency=f0,
                         channel_bandwidth=1.0e6, nchan=pixels.shape[0])
    im["pixels"].data = pixels
    return im


def step_sum_invert(dev, gen, n, count, args):
    rng = numpy.random.default_rng(0)
    pairs = [(image(torch.randn((1, 4, n, n), dtype=torch.float64, device=dev, generator=gen)),
              rng.uniform(0.5, 2.0, (1, 4))) for _ in range(count)]
    pixels = [p[0]["pixels"].data for p in pairs]
    weights = numpy.stack([p[1] for p in pairs])
    sumwt = weights.sum(0)
    out = torch.empty_like(pixels[0])

    def torch_loop():
        acc = torch.zeros_like(pixels[0])
        for x, w in zip(pixels, weights):
            acc += torch.as_tensor(w, device=dev)[..., None, None] * x
        s = torch.as_tensor(sumwt, device=dev)[..., None, None]
        return torch.where(s > 0.0, acc / s, torch.zeros_like(acc))

    flat = [x.reshape(-1) for x in pixels]
    mix_out = out.reshape(1, -1)
    mix_w = weights[:, 0, 0][None, :]
    times = measure({
        "kernel": lambda: kernels.sum_planes(pixels, weights, sumwt, out=out),
        "call": lambda: ih.sum_invert_results(pairs),
        "torch": torch_loop,
        "mix_planes": lambda: kernels.mix_planes(flat, mix_w, mix_out)}, args.warmup, args.repeats)
    nbytes = (count + 1) * out.numel() * 8
    got = ih.sum_invert_results(pairs)[0]["pixels"].data
    equal = bool(torch.equal(got.view(torch.int64), torch_loop().view(torch.int64)))
    ratio = numpy.median(times["mix_planes"]) / numpy.median(times["kernel"])
    report("sum_invert", {"npix": n, "npol": 4, "results": count, "dtype": "float64"}, times,
           {"kernel": nbytes, "call": nbytes, "mix_planes": nbytes},
           {"bit_equal_to_torch": equal, "kernel_bandwidth_over_mix_planes": float(ratio)})


def step_threshold(dev, gen, n, nchan, args):
    cube = torch.randn((nchan, 4, n, n), dtype=torch.float64, device=dev, generator=gen)
    im = image(cube)
    facets = image_scatter_facets(im, facets=8, overlap=max(1, n // 64))

    def torch_path():
        moments = calculate_image_frequency_moments(im)
        return float(torch.amax(torch.abs(moments["pixels"].data[0] / nchan)))

    planes = list(cube)
    mix_out = torch.empty((1, 4, n, n), dtype=torch.float64, device=dev)
    mix_w = numpy.ones((1, nchan))
    times = measure({
        "kernel": lambda: kernels.peak_abs(cube, "moment0"),
        "call": lambda: ih.threshold_list([im], 0.0, 0.1),
        "call_facets": lambda: ih.threshold_list(facets, 0.0, 0.1),
        "torch": torch_path,
        "mix_planes": lambda: kernels.mix_planes(planes, mix_w, mix_out)}, args.warmup, args.repeats)
    read = cube.numel() * 8
    facet_read = sum(f["pixels"].data.numel() for f in facets) * 8
    equal = kernels.peak_abs(cube, "moment0")[0] == torch_path()
    # mix_planes also writes one plane: compare bytes per second, not times
    rate = lambda name, b: b / numpy.median(times[name])
    ratio = rate("kernel", read) / rate("mix_planes", read + mix_out.numel() * 8)
    report("threshold", {"npix": n, "npol": 4, "nchan": nchan, "dtype": "float64",
                         "facets": len(facets), "facet_shape": list(facets[0]["pixels"].data.shape)},
           times, {"kernel": read, "call": read, "call_facets": facet_read,
                   "mix_planes": read + mix_out.numel() * 8},
           {"equal_to_torch": bool(equal), "kernel_bandwidth_over_mix_planes": float(ratio)})


def step_sum_predict(dev, gen, nrows, count, args):
    shape = (nrows, 19306, 64, 4)
    vis = [torch.view_as_complex(torch.randn(shape + (2,), dtype=torch.float32, device=dev,
                                             generator=gen)) for _ in range(count)]
    results = [dm.Visibility.constructor(
        frequency=numpy.linspace(1.0e8, 1.2e8, 64), phasecentre=dm.SkyCoord(0.2, -0.7),
        uvw=numpy.zeros((nrows, 19306, 3)), time=numpy.arange(nrows), vis=v,
        weight=numpy.ones(1), flags=numpy.zeros(1, dtype=int)) for v in vis]

    def torch_loop():
        for v in vis[1:]:
            vis[0] += v

    check = [v[:2].clone() for v in vis]
    ih.sum_predict_results([dm.Visibility.constructor(
        frequency=numpy.linspace(1.0e8, 1.2e8, 64), phasecentre=dm.SkyCoord(0.2, -0.7),
        uvw=numpy.zeros((2, 19306, 3)), time=numpy.arange(2), vis=v, weight=numpy.ones(1),
        flags=numpy.zeros(1, dtype=int)) for v in check])
    want = vis[0][:2].clone()
    for v in vis[1:]:
        want += v[:2]
    equal = bool(torch.equal(torch.view_as_real(check[0]), torch.view_as_real(want)))
    times = measure({"call": lambda: ih.sum_predict_results(results), "torch": torch_loop},
                    args.warmup, args.repeats)
    nbytes = (count + 1) * vis[0].numel() * 8
    report("sum_predict", {"shape": list(shape), "visibilities": count, "dtype": "complex64"},
           times, {"call": nbytes}, {"bit_equal_to_torch": equal})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", default="sum_invert,threshold,sum_predict")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imaging_helpers.py needs a GPU: it measures nothing on the host")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    steps = args.steps.split(",")
    if "sum_invert" in steps:
        step_sum_invert(dev, gen, max(64, int(4096 * args.scale)), 16, args)
        torch.cuda.empty_cache()
    if "threshold" in steps:
        step_threshold(dev, gen, max(64, int(2048 * args.scale)), 16, args)
        torch.cuda.empty_cache()
    if "sum_predict" in steps:
        step_sum_predict(dev, gen, max(2, int(100 * args.scale)), 4, args)


if __name__ == "__main__":
    main()
