"""Time the bandpass resamplers (csrc/bandpass.hip, calibration/
beamformer_utils.resample_bandpass) on one GPU.

Workload: a gain table of 4 times x 512 antennas x 4096 channels x 2 x 2
complex128 (537 MB) onto 384 output channels (the SKA-Low CBF grid across
50-350 MHz), with
  * polyfit at degree 3 on the full band,
  * polyfit at degree 3 with two edges (three segments),
  * interp.

Measured with device events, after warm-up calls, median of the repeats:
  * the kernel alone: the C entry point on tables that are already on the
    device and an output that is already allocated;
  * the whole resample_bandpass call on a device-tensor table (the host
    tables in longdouble, their upload, the allocation and the kernel), also
    by a host clock around a device synchronise;
  * kernels.mix_planes over the same bytes in the same session, as the
    streaming yardstick: 11 input planes into 1 output plane, sized so that it
    reads what the resampler reads and writes 1/11 of it (the resampler
    writes 384/4096);
  * the host path the kernels replace: numpy.polynomial.polyfit on the real
    and on the imaginary part plus polyval (or numpy.interp) per spectrum, on
    a sample of the spectra, extrapolated to all of them.
Prints JSON lines.  cubicspl has no kernel of its own and is not timed here.

  python scripts/bench_bandpass.py [--times 4] [--ants 512] [--chan 4096] [--sample 64]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from numpy.polynomial import polynomial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-python_amd"))

from ska_sdp_func_python_amd import _lib, kernels  # noqa: E402
from ska_sdp_func_python_amd import datamodels as dm  # noqa: E402
from ska_sdp_func_python_amd.calibration import beamformer_utils as bu  # noqa: E402


def event_ms(fn, warmup, repeats):
    """Median device-event and host-clock milliseconds of fn(), its last result
    and the smallest and largest device-event time."""
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
    return float(np.median(dev_ms)), float(np.median(host_ms)), out, [min(dev_ms), max(dev_ms)]


def host_spectrum(alg, f_out, f_in, spectrum, edges, deg):
    """One spectrum as the reference resamples it (beamformer_utils.py:389-461)."""
    if alg == "interp":
        return np.interp(f_out, f_in, spectrum)
    out = np.empty(len(f_out), complex)
    df = f_in[1] - f_in[0]
    for k in range(len(edges) - 1):
        ch = slice(edges[k], edges[k + 1])
        sel = (f_out >= f_in[edges[k]] - df / 2) & (f_out < f_in[edges[k + 1] - 1] + df / 2)
        re = polynomial.polyfit(f_in[ch], spectrum[ch].real, deg)
        im = polynomial.polyfit(f_in[ch], spectrum[ch].imag, deg)
        out[sel] = polynomial.polyval(f_out[sel], re) + 1j * polynomial.polyval(f_out[sel], im)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--times", type=int, default=4)
    ap.add_argument("--ants", type=int, default=512)
    ap.add_argument("--chan", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=64, help="spectra of the host path that are run")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bandpass.py needs a GPU: it measures nothing on the host alone")
    dev = torch.device("cuda:0")
    nt, na, c_in = args.times, args.ants, args.chan
    f_in = np.linspace(50e6, 350e6, c_in)
    torch.manual_seed(0)
    x = torch.linspace(0, 1, c_in, dtype=torch.float64, device=dev)[None, None, :, None, None]
    lead = (nt, na, 1, 2, 2)
    amp = 1 + 0.1 * torch.rand(lead, dtype=torch.float64, device=dev) * torch.cos(3 * x)
    phase = 6 * torch.rand(lead, dtype=torch.float64, device=dev) * x \
        + 0.05 * torch.randn((nt, na, c_in, 2, 2), dtype=torch.float64, device=dev)
    gain = torch.polar(amp.expand_as(phase).contiguous(), phase)
    gt = dm.GainTable.constructor(
        gain, np.arange(nt) * 10.0, np.full(nt, 10.0), torch.ones_like(phase),
        torch.zeros((nt, c_in, 2, 2), dtype=torch.float64, device=dev), f_in,
        dm.PolarisationFrame("linear"), None, dm.Configuration("LOW"), "B")
    f_out = bu.set_beamformer_frequencies(gt)
    c_out = len(f_out)
    in_bytes, out_bytes = gain.numel() * 16, nt * na * c_out * 4 * 16
    nspec = nt * na * 4
    runs = [("polyfit", "polyfit_deg3", None, 3),
            ("polyfit", "polyfit_deg3_2edges", [c_in // 3, 2 * c_in // 3], 3),
            ("interp", "interp", None, None)]
    results = {}
    for alg, name, edges, deg in runs:
        out = torch.empty((nt, na, c_out, 2, 2), dtype=torch.complex128, device=dev)
        if alg == "polyfit":
            q, e, seg, ed = bu.polyfit_tables(f_out, f_in, edges, deg)
            tabs = [torch.as_tensor(a, device=dev) for a in (q, e, seg, ed)]
            call = lambda: _lib.call(  # noqa: E731
                "sdp_hip_resample_polyfit", nt * na, c_in, c_out, 2, deg, len(ed) - 1,
                kernels.ptr(gain), kernels.ptr(out), *[kernels.ptr(t) for t in tabs],
                kernels.stream(dev))
        else:
            tabs = [torch.as_tensor(a, device=dev)
                    for a in (f_in, f_out, bu.interp_intervals(f_out, f_in))]
            call = lambda: _lib.call(  # noqa: E731
                "sdp_hip_resample_interp", nt * na, c_in, c_out, 2, kernels.ptr(gain),
                kernels.ptr(out), *[kernels.ptr(t) for t in tabs], kernels.stream(dev))
        k_ms, _, _, k_range = event_ms(call, args.warmup, args.repeats)
        kw = dict(edges=edges, polydeg=deg) if alg == "polyfit" else {}
        w_dev, w_host, whole, w_range = event_ms(
            lambda: bu.resample_bandpass(f_out, gt, alg=alg, **kw), 1, args.repeats)
        assert torch.equal(torch.view_as_real(whole), torch.view_as_real(out))
        # interp reads two knots per output point, not the whole table
        moved = in_bytes + out_bytes if alg == "polyfit" else None
        results[name] = k_ms
        print(json.dumps({
            "op": name, "shape": [nt, na, c_in, 2, 2], "c_out": c_out, "kernel_ms": k_ms,
            "kernel_ms_min_max": k_range,
            "kernel_GBps_of_table_read_plus_written": moved and moved / k_ms / 1e6,
            "whole_call_device_event_ms": w_dev, "whole_call_ms_min_max": w_range,
            "whole_call_host_clock_ms": w_host}), flush=True)
        del out, whole

    # ---- the streaming yardstick on the same bytes ----
    nin = 11
    npix = in_bytes // 8 // nin
    planes = torch.view_as_real(gain).reshape(-1)[:nin * npix].reshape(nin, npix)
    mixed = torch.empty((1, npix), dtype=torch.float64, device=dev)
    weights = np.full((1, nin), 1.0 / nin)
    m_ms, _, _, m_range = event_ms(lambda: kernels.mix_planes(planes, weights, mixed),
                                   args.warmup, args.repeats)
    m_bytes = (nin + 1) * npix * 8
    print(json.dumps({"op": "mix_planes", "nin": nin, "nout": 1, "npix": npix, "device_ms": m_ms,
                      "device_ms_min_max": m_range,
                      "GBps": m_bytes / m_ms / 1e6,
                      "polyfit_deg3_kernel_over_mix_planes": results["polyfit_deg3"] / m_ms}),
          flush=True)

    # ---- the host path, on a sample of spectra ----
    rng = np.random.default_rng(0)
    pick = rng.integers(0, nt * na, args.sample)
    rows = gain.reshape(nt * na, c_in, 2, 2)[torch.as_tensor(pick, device=dev)].cpu().numpy()
    for alg, name, edges, deg in runs:
        ed = bu.normalise_edges(edges, c_in) if alg == "polyfit" else None
        t0 = time.perf_counter()
        for r in range(len(pick)):
            host_spectrum(alg, f_out, f_in, rows[r, :, r % 2, (r // 2) % 2], ed, deg)
        ms = 1e3 * (time.perf_counter() - t0)
        total = ms / len(pick) * nspec
        print(json.dumps({"op": f"host_{name}", "sample": len(pick), "ms_per_spectrum":
                          ms / len(pick), "extrapolated_total_ms": total,
                          "extrapolated_over_kernel": total / results[name]}), flush=True)


if __name__ == "__main__":
    main()
