"""The beamformer fixtures (tests/golden/beamformer_*.npz, written by
tests/golden/make_golden_beamformer.py) as objects, and the bounds that both
tests/test_beamformer_cpu.py and tests/test_gpu_beamformer.py hold results to.

Bounds (eps = 2^-52; none of them comes from what the code under test gives):
  polyfit   against the reference: 2 S_case + (n_seg + 2 deg + 8) eps
            sum_c |M[co, c]| |g_c|; against the tight restatement the second
            term alone.  M is the tight restatement's operator row, S_case the
            reference's own distance from the tight restatement (stored in the
            fixture).  The second term is the rounding bound of the dot
            products the kernel makes, the first the reference's error doubled.
  cubicspl  against the reference: (C_in + 8) eps sum_c |M[co, c]| |g_c|, M
            built by scipy.
  interp    equal bits.
  matrix product  |d_ij| <= 4 eps (|A| |B|)_ij: the a-priori bound of a
            two-term complex dot product, about 3.3 u, with a margin.
"""

import functools
import os

import numpy as np

import bandpass_restatement as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = br.EPS
RESAMPLE = ("wide", "narrow", "mid", "deg5", "edges", "lowband")
MULTIPLY = ("G1xB5", "B5xD5", "B5xG1", "B5xG1_elem", "Gs1xBs5", "B5xB5b")


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(GOLDEN, f"beamformer_{name}.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def table(gain, frequency, jones_type="B", name="LOW-AA0.5", weight=None, residual=None,
          convert=None):
    """A GainTable over copies of the arrays; ``convert`` (numpy -> tensor)
    puts gain, weight and residual on the device."""
    from ska_sdp_func_python_amd import datamodels as dm
    gain = np.array(gain)
    nt, _, nchan, nrec, _ = gain.shape
    weight = np.ones(gain.shape) if weight is None else np.array(weight)
    residual = np.zeros((nt, nchan, nrec, nrec)) if residual is None else np.array(residual)
    c = convert or (lambda a: a)
    return dm.GainTable.constructor(
        c(gain), 100.0 + 10.0 * np.arange(nt), np.full(nt, 10.0), c(weight), c(residual),
        np.array(frequency, dtype=float), dm.PolarisationFrame("stokesI" if nrec == 1 else "linear"),
        dm.SkyCoord(0.0, -0.8), dm.Configuration(name), jones_type)


def multiply_table(g, key, convert=None):
    return table(g[f"{key}_gain"], g[f"{key}_frequency"], str(g[f"{key}_jones"]),
                 weight=g[f"{key}_weight"], residual=g[f"{key}_residual"], convert=convert)


def product_bound(a, b):
    """4 eps (|A| |B|)_ij with the single-channel table broadcast."""
    return 4 * EPS * (np.abs(a)[..., :, :, None] * np.abs(b)[..., None, :, :]).sum(-2)


def resample_args(g):
    """(edges, polydeg) as the fixture's call passed them."""
    edges = [int(v) for v in g["edges"]] or None
    deg = int(g["polydeg"])
    return edges, (None if deg < 0 else deg)


@functools.lru_cache(maxsize=None)
def polyfit_yardstick(case):
    """(tight result, rounding bound, reference bound, outside mask) of a
    resample fixture; computed once and shared."""
    g = load(f"resample_{case}")
    edges, deg = resample_args(g)
    deg = 3 if deg is None else deg
    return polyfit_yardstick_of(g["frequency_out"], g["frequency"], g["gain"], edges, deg,
                                float(g["s_polyfit"]))


def polyfit_yardstick_of(freq_out, freq_in, gain, edges, deg, s_case=0.0):
    m, seg = br.tight_operator(freq_out, freq_in, edges, deg)
    nseg = len(br.normalise_edges(edges, len(freq_in))) - 1
    rounding = (nseg + 2 * deg + 8) * EPS * br.operator_scale(m, gain)
    return br.apply_operator(m, gain, seg), rounding, 2 * s_case + rounding, seg < 0


@functools.lru_cache(maxsize=None)
def spline_bound(case):
    from scipy.interpolate import CubicSpline
    g = load(f"resample_{case}")
    f = g["frequency"]
    m = CubicSpline(f, np.eye(len(f)))(g["frequency_out"])
    return (len(f) + 8) * EPS * br.operator_scale(m, g["gain"])


def check_polyfit(case, got, label):
    """Hold a polyfit result to both yardsticks; prints the DEV line."""
    g = load(f"resample_{case}")
    tight, rounding, ref_bound, outside = polyfit_yardstick(case)
    got = np.asarray(got)
    inside = ~outside
    assert np.all(np.isnan(got[:, :, outside].real)) and np.all(np.isnan(got[:, :, outside].imag))
    d_tight = np.abs(got - tight)[:, :, inside]
    d_ref = np.abs(got - g["out_polyfit"])[:, :, inside]
    print(f"DEV {label} polyfit {case}: vs tight {d_tight.max():.2e} "
          f"({(d_tight / rounding[:, :, inside]).max():.3f} of bound), vs reference "
          f"{d_ref.max():.2e} ({(d_ref / ref_bound[:, :, inside]).max():.3f} of bound)")
    assert np.all(d_tight <= rounding[:, :, inside])
    assert np.all(d_ref <= ref_bound[:, :, inside])


def check_spline(case, got, label):
    g = load(f"resample_{case}")
    bound = spline_bound(case)
    d = np.abs(np.asarray(got) - g["out_cubicspl"])
    print(f"DEV {label} cubicspl {case}: {d.max():.2e} ({(d / bound).max():.3f} of bound)")
    assert np.all(d <= bound)


def same_bits(a, b):
    """Equal shape, dtype and bits of every real and imaginary part (-0.0 is
    not +0.0); a NaN matches a NaN whatever its payload."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    fa, fb = a.view(np.float64).ravel(), b.view(np.float64).ravel()
    nan = np.isnan(fa)
    return bool(np.array_equal(nan, np.isnan(fb))
                and np.array_equal(fa[~nan].view(np.uint64), fb[~nan].view(np.uint64)))
