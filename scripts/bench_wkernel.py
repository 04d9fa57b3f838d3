"""Time the creation of w-projection convolution functions
(csrc/wkernel.hip through grid_data/convolution_functions.py) on one GPU.

One shape: a 4096 x 4096 image with cells of 5e-5 rad, far field of 256
pixels, oversampling 8, support 32, 65 w planes 50 wavelengths apart -- 65 x
9 x 9 kernels of 32 x 32, 86 MB of complex128.

  create   create_awterm_convolutionfunction on an image whose pixels are on
           the device (the whole call: host checks, WCS, grid correction,
           taper upload, kernels, normalisation)
  kernel   kernels.wkernel_create alone (twiddles, far fields, both products)
  torch    the recipe transcribed to torch operations on the device: the far
           fields filled, padded to 2048 x 2048, torch.fft.ifft2 between
           shifts in chunks of planes that fit, one strided gather per chunk
  host     the recipe in numpy with fourier_transforms on the host for 3
           planes, wall clock, extrapolated to the 65

create, kernel and torch alternate; every call is timed with device events
after warm-up calls.  Medians with min and max go to one JSON line, with the
largest difference between create's and torch's results relative to the peak.

  python scripts/bench_wkernel.py [--repeats 11] [--warmup 2] [--chunk 13]
"""

import argparse
import json
import math
import os
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-python_amd"))

from ska_sdp_func_python_amd import datamodels as dm  # noqa: E402
from ska_sdp_func_python_amd import fourier_transforms as ft  # noqa: E402
from ska_sdp_func_python_amd import kernels  # noqa: E402
from ska_sdp_func_python_amd.grid_data import create_awterm_convolutionfunction  # noqa: E402

NPIXEL, CELL = 4096, 5e-5
N, OS, SUPPORT, NW, WSTEP = 256, 8, 32, 65, 50.0
H = OS // 2
ND = 2 * H + 1


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


def torch_recipe(dev, fov, ws, taper, chunk):
    """w_beam -> taper -> pad_mid -> ifft -> extract_oversampled, as torch
    operations; not normalised.  [nw, nd, nd, support, support]."""
    npad = OS * N
    c = (torch.arange(N, device=dev, dtype=torch.float64) - N // 2) / N
    r2 = fov**2 * (c[:, None] ** 2 + c[None, :] ** 2)
    chirp = 1 - torch.sqrt(1.0 - r2)
    tt = taper[:, None] * taper[None, :]
    c0 = npad // 2 - OS * (SUPPORT // 2)
    start = c0 - (torch.arange(ND, device=dev) - H)
    idx = start[:, None] + OS * torch.arange(SUPPORT, device=dev)[None, :]      # [nd, support]
    rows, cols = idx[:, None, :, None], idx[None, :, None, :]
    out = torch.empty((len(ws), ND, ND, SUPPORT, SUPPORT), dtype=torch.complex128, device=dev)
    pad = npad // 2 - N // 2
    for z0 in range(0, len(ws), chunk):
        w = torch.as_tensor(ws[z0:z0 + chunk], dtype=torch.float64, device=dev)
        ph = (-2 * math.pi * -w)[:, None, None] * chirp
        far = torch.polar(tt.expand_as(ph).contiguous(), ph)
        parent = ft.ifft(torch.nn.functional.pad(far, (pad, pad, pad, pad))[:, None])[:, 0]
        out[z0:z0 + chunk] = OS * OS * parent[:, rows, cols]
    return out


def host_recipe(fov, ws):
    """The recipe in numpy for the planes ``ws``."""
    t = ft.grdsf(numpy.abs(2 * ft.coordinates(N)))[0]
    out = numpy.zeros((len(ws), ND, ND, SUPPORT, SUPPORT), complex)
    c0 = OS * N // 2 - OS * (SUPPORT // 2)
    for z, w in enumerate(ws):
        parent = ft.ifft(ft.pad_mid(ft.w_beam(N, fov, -w) * numpy.outer(t, t), OS * N))
        for iv in range(ND):
            for iu in range(ND):
                my, mx = c0 - (iv - H), c0 - (iu - H)
                out[z, iv, iu] = OS * OS * parent[my:my + OS * SUPPORT:OS, mx:mx + OS * SUPPORT:OS]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--chunk", type=int, default=13, help="planes per FFT batch of the torch path")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wkernel.py needs a GPU")
    dev = torch.device("cuda:0")
    im = dm.create_image(NPIXEL, CELL, dm.SkyCoord(0.2, -0.7), frequency=1.0e8,
                         channel_bandwidth=1.0e6)
    im["pixels"].data = torch.zeros((1, 1, NPIXEL, NPIXEL), dtype=torch.float64, device=dev)
    fov = NPIXEL * float(numpy.deg2rad(abs(im.image_acc.wcs.wcs.cdelt[1])))
    ws = [(z - NW // 2) * WSTEP for z in range(NW)]
    w_dev = torch.as_tensor(ws, dtype=torch.float64, device=dev)
    taper = torch.as_tensor(ft.grdsf(numpy.abs(2 * ft.coordinates(N)))[0], device=dev)
    kw = dict(nw=NW, wstep=WSTEP, oversampling=OS, support=SUPPORT, farfield_npixel=N,
              normalise=False)

    times = measure({
        "create": lambda: create_awterm_convolutionfunction(im, **kw),
        "kernel": lambda: kernels.wkernel_create(N, OS, SUPPORT, w_dev, fov, taper=taper),
        "torch": lambda: torch_recipe(dev, fov, ws, taper, args.chunk)}, args.warmup, args.repeats)

    got = create_awterm_convolutionfunction(im, **kw)[1]["pixels"].data[0, 0]
    want = torch_recipe(dev, fov, ws, taper, args.chunk)
    diff = float((got - want).abs().max() / want.abs().max())
    t0 = time.perf_counter()
    host = host_recipe(fov, ws[NW // 2:NW // 2 + 3])
    host_s = (time.perf_counter() - t0) * NW / 3
    host_diff = float(numpy.abs(got[NW // 2:NW // 2 + 3].cpu().numpy() - host).max()
                      / numpy.abs(host).max())

    out = {"step": "wkernel", "image": NPIXEL, "cell": CELL, "farfield_npixel": N,
           "oversampling": OS, "support": SUPPORT, "nw": NW, "wstep": WSTEP,
           "cf_bytes": got.numel() * 16, "torch_chunk": args.chunk}
    for name, ms in times.items():
        out[name] = {"ms_median": float(numpy.median(ms)), "ms_min": min(ms), "ms_max": max(ms),
                     "n": len(ms)}
    out["host_numpy_s_extrapolated_from_3_planes"] = host_s
    out["torch_over_create"] = out["torch"]["ms_median"] / out["create"]["ms_median"]
    out["host_over_create"] = host_s * 1e3 / out["create"]["ms_median"]
    out["create_vs_torch_max_rel_diff"] = diff
    out["create_vs_host_max_rel_diff"] = host_diff
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
