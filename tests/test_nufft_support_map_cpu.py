"""The epsilon -> kernel support map and the w-plane layout of the HIP plan
(sdp_hip_wstack_layout: no device work) against oracle/wgrid_cpu, the host
restatement whose errors bound the GPU sweep of
tests/test_gpu_nufft_supports.py.

The documented rule is W = ceil(-log10(epsilon / 10)), clamped to [2, 8] on the
fp32 path (epsilon >= 1e-7) and to [9, 16] on the fp64 path.  Checked at
every decade 1e-1 .. 1e-15, a hair on either side of each (1e-k (1 +- 1e-6)),
between decades and outside the supported range."""

import numpy as np
import pytest

import wgrid_cpu

C_LIGHT = 299792458.0
DECADES = [(float(f"1e-{k}"), k + 1) for k in range(1, 16)]
# (epsilon, W by the documented rule before clamping)
EPS_W = (DECADES
         + [(e * (1.0 + 1e-6), W) for e, W in DECADES]   # a hair above the decade: same W
         + [(e * (1.0 - 1e-6), W + 1) for e, W in DECADES]  # a hair below: one more
         + [(3e-4, 5), (2e-13, 14), (5e-8, 9), (1.0, 1), (0.5, 2), (1e-18, 19)])

# {wmin, wmax, umax, vmax, fmin, fmax} (metres, Hz), image and pixel sizes
LAYOUTS = {
    "wide": ([-59000.0 * 0.25, 61000.0 * 0.25, 480.0, 470.0, 1.0e9, 1.2e9], 64, 48, 2.25e-4, 2.025e-4),
    "one_w": ([5321.7, 5321.7, 300.0, 200.0, 1.1e9, 1.1e9], 64, 48, 2.25e-4, 2.025e-4),
    "positive": ([1.0e5, 4.3e5, 3000.0, 3500.0, C_LIGHT, C_LIGHT], 64, 64, 2.0 ** -13, 2.0 ** -13),
}


def _clamped(eps, W):
    return min(max(W, 2), 8) if eps >= 1e-7 else min(max(W, 9), 16)


def _oracle_layout(bounds, nx, ny, px, py, eps, dow):
    """wgrid_cpu's support and plane count for two rows that realise `bounds`."""
    wmin, wmax, umax, vmax, fmin, fmax = bounds
    uvw = np.array([[umax, -vmax, wmin], [-umax, vmax, wmax]])
    freq = np.array([fmin, fmax]) if fmax > fmin else np.array([fmin])
    info = {}
    wgrid_cpu.ms2dirty(uvw, freq, np.ones((2, freq.size), np.complex128), None, nx, ny, px, py,
                       eps, dow, nthreads=1, precision="double" if eps < 1e-7 else "single",
                       info=info)
    return info


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("dow", [False, True])
def test_support_map_and_planes_match_the_restatement(layout, dow):
    from ska_sdp_func_python_amd import kernels
    bounds, nx, ny, px, py = LAYOUTS[layout]
    for eps, W_rule in EPS_W:
        lay = kernels.wstack_layout(bounds, nx, ny, px, py, eps, dow)
        ref = _oracle_layout(bounds, nx, ny, px, py, eps, dow)
        assert lay["support"] == ref["support"] == _clamped(eps, W_rule), (eps, lay, ref)
        assert lay["fp64"] == (1 if eps < 1e-7 else 0), eps
        assert lay["nplanes"] == ref["nplanes"], (eps, lay, ref)
        assert lay["beta"] == pytest.approx(2.30 * lay["support"], rel=1e-7)
        if not dow:
            assert lay["nplanes"] == 1
        elif layout == "one_w":
            assert lay["nplanes"] == lay["support"]  # wmin == wmax: a single first plane
        else:
            assert lay["nplanes"] - lay["support"] + 1 >= 6


def test_flipped_w_gives_the_mirrored_layout():
    """flip_uw negates w: the layout of the mirrored bounds, same planes."""
    from ska_sdp_func_python_amd import kernels
    bounds, nx, ny, px, py = LAYOUTS["positive"]
    mirrored = [-bounds[1], -bounds[0]] + bounds[2:]
    for eps, _ in DECADES:
        a = kernels.wstack_layout(bounds, nx, ny, px, py, eps, True, flip_uw=True)
        b = kernels.wstack_layout(mirrored, nx, ny, px, py, eps, True)
        assert (a["support"], a["nplanes"], a["w0"], a["dw"]) == \
               (b["support"], b["nplanes"], b["w0"], b["dw"]), eps


def test_precision_fp32_keeps_the_fp32_supports():
    from ska_sdp_func_python_amd import kernels
    bounds, nx, ny, px, py = LAYOUTS["wide"]
    for eps in (1e-8, 1e-12, 1e-18):
        lay = kernels.wstack_layout(bounds, nx, ny, px, py, eps, True, precision="fp32")
        assert lay["fp64"] == 0 and lay["support"] == 8
