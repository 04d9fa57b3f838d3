"""Time the complex Hogbom minor cycle (csrc/clean.hip, k_select_c /
k_update_c) on one GPU, beside the real Hogbom cycle and the host path.

Workload: one Stokes Q / U pair of 4096 x 4096 float64: 60 polarised point
sources of random angle convolved with a PSF of unit peak (a Gaussian core on
slowly decaying rings), on noise of 0.01.  200 cycles at gain 0.1 with both
thresholds 0, so that every cycle runs.

Measured in one session with device events around the library call, after a
warm-up call, the median of the repeats with (min - max):
  * kernels.clean_plane_complex on the pair, with the full PSF and with the
    512 x 512 box that bound_psf_list cuts for psf_support=256;
  * kernels.clean_plane("hogbom") on the Q plane and on the U plane, one after
    the other: the device alternative that ignores the Q-U coupling;
  * the host path the feature replaces: the copy of both planes to the host,
    once, and the numpy restatement (tests/hogbom_complex_restatement.py) for
    a handful of cycles by a host clock.  The device's planes after as many
    cycles are compared with the restatement's.
Every timed call starts from a fresh copy of the dirty planes, made outside
the timed window.  Prints JSON lines.

  python scripts/bench_hogbom_complex.py [--npix 4096] [--cycles 200] [--host-cycles 5]
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

import hogbom_complex_restatement as hr  # noqa: E402
from ska_sdp_func_python_amd import kernels  # noqa: E402


def event_ms(setup, fn, warmup, repeats):
    """Device-event milliseconds of fn(setup()) -- median, min, max -- and its last result."""
    times, out = [], None
    for i in range(warmup + repeats):
        state = setup()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(state)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times)), out


def make_inputs(n, dev):
    d = torch.arange(n, dtype=torch.float64, device=dev) - n // 2
    r = torch.sqrt(d[:, None] ** 2 + d[None, :] ** 2)
    psf = torch.exp(-r ** 2 / 18.0) + 0.05 * torch.cos(0.3 * r) * torch.exp(-r / 300.0)
    psf = psf / psf.max()
    rng = np.random.default_rng(0)
    model = torch.zeros((2, n, n), dtype=torch.float64, device=dev)
    for _ in range(60):
        y, x = (int(v) for v in rng.integers(n // 8, n - n // 8, 2))
        p, chi = rng.uniform(0.3, 1.0), rng.uniform(0.0, np.pi)
        model[0, y, x], model[1, y, x] = p * np.cos(2 * chi), p * np.sin(2 * chi)
    kernel = torch.fft.fft2(torch.fft.ifftshift(psf))
    dirty = torch.fft.ifft2(torch.fft.fft2(model) * kernel).real
    torch.manual_seed(0)
    dirty = (dirty + 0.01 * torch.randn((2, n, n), dtype=torch.float64, device=dev)).contiguous()
    return dirty, psf.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npix", type=int, default=4096)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--host-cycles", type=int, default=5)
    ap.add_argument("--psf-support", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hogbom_complex.py needs a GPU: it measures nothing on the host alone")
    dev = torch.device("cuda:0")
    n, cycles, gain = args.npix, args.cycles, 0.1
    dirty, psf = make_inputs(n, dev)
    c, s = n // 2, args.psf_support
    boxes = {"full": psf, f"box{2 * s}": psf[c - s:c + s, c - s:c + s].contiguous()}

    def fresh():
        return dirty.clone(), torch.zeros_like(dirty)

    def complex_clean(box, niter=cycles):
        def run(state):
            res, comps = state
            return kernels.clean_plane_complex(res, box, comps, gain, 1.0, 0.0, niter), res, comps
        return run

    def real_twice(box):
        def run(state):
            res, comps = state
            return [kernels.clean_plane("hogbom", res[p:p + 1], box[None, None], comps[p], gain, 1.0,
                                        0.0, cycles) for p in range(2)]
        return run

    for tag, box in boxes.items():
        for op, fn in (("hogbom_complex", complex_clean(box)), ("hogbom_real_q_then_u", real_twice(box))):
            med, lo, hi, out = event_ms(fresh, fn, args.warmup, args.repeats)
            # a "cycle" of the real pair is one Q cycle and one U cycle
            done = out[0][0] if op == "hogbom_complex" else [o[0] for o in out]
            print(json.dumps({"op": op, "npix": n, "psf": tag, "psf_shape": list(box.shape),
                              "cycles": done, "device_ms_median": med, "device_ms_min": lo,
                              "device_ms_max": hi, "ms_per_cycle": med / cycles,
                              "ms_per_cycle_min": lo / cycles, "ms_per_cycle_max": hi / cycles,
                              "repeats": args.repeats}), flush=True)

    # ---- the host path: copy both planes, a handful of numpy cycles ----
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = dirty.cpu().numpy()
    copy_ms = 1e3 * (time.perf_counter() - t0)
    host_psf = psf.cpu().numpy()
    t0 = time.perf_counter()
    want = hr.hogbom_complex(host[0], host[1], host_psf, None, gain, 0.0, args.host_cycles, 0.0)
    host_ms = 1e3 * (time.perf_counter() - t0)
    _, res, comps = complex_clean(psf, args.host_cycles)(fresh())
    same = bool(np.array_equal(res.cpu().numpy(), np.stack(want[2:4]))
                and np.array_equal(comps.cpu().numpy(), np.stack(want[0:2])))
    print(json.dumps({"op": "host_restatement", "npix": n, "psf": "full", "copy_to_host_ms": copy_ms,
                      "cycles": args.host_cycles, "host_clock_ms": host_ms,
                      "ms_per_cycle": host_ms / args.host_cycles,
                      "device_equals_restatement": same}), flush=True)


if __name__ == "__main__":
    main()
