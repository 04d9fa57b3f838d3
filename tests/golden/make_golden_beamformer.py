"""Generate the beamformer-utility fixtures (tests/golden/beamformer_*.npz)
from the REFERENCE's own code.

Run where the reference sources are (they never travel to the GPU box):
    python tests/golden/make_golden_beamformer.py

As make_golden_chain.py: the four functions and three classes of the
reference's calibration/beamformer_utils.py are AST-extracted and executed
over the datamodels shim.  Only inputs and outputs are stored.

Fixtures (tests/beamformer_cases.py rebuilds the tables from them):
  beamformer_expand       3 times x 4 antennas x 2 x 2 "K" table onto 5
                          frequencies, reference_to_centre both ways
  beamformer_multiply     G (1 channel) x B (5), B x D with leakage, B x G,
                          B x G elementwise, 1 x 1 tables, every refusal
  beamformer_frequencies  LOW and MID grids, one channel, unknown array
  beamformer_resample_*   noisy smooth spectra through polyfit, cubicspl and
                          interp: wide, narrow, mid, deg5, edges, lowband

The resample cases must be a yardstick: on each the scaled Vandermonde matrix
that numpy's polyfit decomposes has a smallest / largest singular value of at
least 10 x numpy's rcond = n eps, and no RankWarning is raised; the generator
refuses to store a case that breaks this.  Per case it stores
S = max |reference - tight restatement| (tests/bandpass_restatement.py), the
reference's own distance from the exact least-squares polynomial.
"""

import ast
import logging
import os
import sys
import warnings

import numpy as np
from numpy.polynomial import polynomial
from scipy import interpolate

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import REF, dm, save  # noqa: E402

import bandpass_restatement as br  # noqa: E402

NAMES = ["set_beamformer_frequencies", "expand_delay_phase", "_set_gaintable_product_shape",
         "multiply_gaintable_jones", "resample_bandpass", "PolynomialInterpolator",
         "NumpyLinearInterpolator", "ScipySplineInterpolator"]


def reference():
    with open(os.path.join(REF, "calibration/beamformer_utils.py")) as f:
        tree = ast.parse(f.read())
    defs = [n for n in tree.body
            if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in NAMES]
    assert {d.name for d in defs} == set(NAMES)
    ns = {"numpy": np, "polynomial": polynomial, "interpolate": interpolate,
          "GainTable": dm.GainTable, "log": logging.getLogger("reference")}
    exec(compile(ast.Module(body=defs, type_ignores=[]), "beamformer_utils.py", "exec"), ns)
    return ns


def table(gain, frequency, jones_type, name="LOW-AA0.5", seed=0):
    rng = np.random.default_rng(seed)
    nt, na, nchan, nrec, _ = gain.shape
    return dm.GainTable.constructor(
        gain, 100.0 + 10.0 * np.arange(nt), np.full(nt, 10.0),
        rng.uniform(0.5, 2.0, gain.shape), rng.uniform(0.0, 0.1, (nt, nchan, nrec, nrec)),
        frequency, dm.PolarisationFrame("stokesI" if nrec == 1 else "linear"),
        dm.SkyCoord(0.0, -0.8), dm.Configuration(name), jones_type)


def arr(x):
    return np.asarray(getattr(x, "data", x)).copy()


def make_expand(ref):
    rng = np.random.default_rng(11)
    gain = np.exp(1j * rng.uniform(-np.pi, np.pi, (3, 4, 1, 2, 2)))
    gt = table(gain, [1.5e8], "K")
    frequency = np.linspace(1.2e8, 1.8e8, 5)
    out = dict(gain=gain, frequency0=np.array([1.5e8]), frequency=frequency)
    for tag, centre in (("centre", True), ("raw", False)):
        keep = frequency.copy()
        got = ref["expand_delay_phase"](gt, frequency, reference_to_centre=centre)
        assert np.array_equal(keep, frequency) and got.jones_type == "B"
        assert np.all(arr(got["weight"]) == 1) and np.all(arr(got["residual"]) == 0)
        out[f"out_{tag}"] = arr(got["gain"])
    for name, bad in (("type", table(gain, [1.5e8], "B")),
                      ("frequency", table(np.repeat(gain, 2, 2), [1.5e8, 1.6e8], "K"))):
        try:
            ref["expand_delay_phase"](bad, frequency)
            raise AssertionError(name)
        except ValueError as e:
            out[f"error_{name}"] = np.array(str(e)[:12])
    save("beamformer_expand.npz", **out)


def make_multiply(ref):
    rng = np.random.default_rng(12)
    freq5 = np.linspace(1.0e8, 1.1e8, 5)

    def jones(nchan, nrec, kind, nt=3, na=4):
        shape = (nt, na, nchan, nrec, nrec)
        g = rng.normal(1.0, 0.1, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))
        if nrec == 2 and kind == "G":      # G: diagonal; B and D: full matrices
            g[..., 0, 1] = g[..., 1, 0] = 0
        if nrec == 2 and kind == "B":
            g[..., 0, 1] *= 0.05
            g[..., 1, 0] *= 0.05
        if kind == "D":
            g[..., 0, 0] = g[..., 1, 1] = 1
            g[..., 0, 1] *= 0.05
            g[..., 1, 0] *= 0.05
        f = freq5 if nchan == 5 else [1.05e8]
        return table(g, f, kind, seed=int(rng.integers(1 << 30)))

    tabs = {"G1": jones(1, 2, "G"), "B5": jones(5, 2, "B"), "D5": jones(5, 2, "D"),
            "Gs1": jones(1, 1, "G"), "Bs5": jones(5, 1, "B"), "B5b": jones(5, 2, "B")}
    out = {}
    for k, t in tabs.items():
        for v in ("gain", "weight", "residual", "frequency"):
            out[f"{k}_{v}"] = arr(t[v])
        out[f"{k}_jones"] = np.array(t.jones_type)
    runs = {"G1xB5": ("G1", "B5", False), "B5xD5": ("B5", "D5", False),
            "B5xG1": ("B5", "G1", False), "B5xG1_elem": ("B5", "G1", True),
            "Gs1xBs5": ("Gs1", "Bs5", False), "B5xB5b": ("B5", "B5b", False)}
    for k, (a, b, elem) in runs.items():
        got = ref["multiply_gaintable_jones"](tabs[a], tabs[b], elementwise=elem)
        out[f"run_{k}"] = np.array([a, b, str(int(elem))])
        for v in ("gain", "weight", "residual", "frequency"):
            out[f"{k}_out_{v}"] = arr(got[v])
        out[f"{k}_out_jones"] = np.array(got.jones_type)
    refusals = {
        "K": (table(arr(tabs["G1"]["gain"]), [1.05e8], "K"), tabs["B5"], False),
        "time": (jones(5, 2, "B", nt=2), tabs["B5"], False),
        "antenna": (jones(5, 2, "B", na=3), tabs["B5"], False),
        "frequency": (table(np.repeat(arr(tabs["G1"]["gain"]), 3, 2), freq5[:3], "B"), tabs["B5"],
                      False),
        "pol": (tabs["Bs5"], tabs["B5"], True),
        "matrix": (tabs["B5"], tabs["Bs5"], False),
    }
    for k, (a, b, elem) in refusals.items():
        try:
            ref["multiply_gaintable_jones"](a, b, elementwise=elem)
            raise AssertionError(k)
        except ValueError as e:
            out[f"error_{k}"] = np.array(str(e)[:10])
    save("beamformer_multiply.npz", **out)


def make_frequencies(ref):
    out = {}
    cases = {"low": ("LOW-AA0.5", np.linspace(0.8e8, 1.2e8, 5), None),
             "mid": ("MID", 1.0e9 + 7.0e3 * np.arange(100), None),
             "one": ("LOW-AA0.5", np.array([1.0e8]), None),
             "unknown": ("ASKAP", np.linspace(0.8e8, 1.2e8, 5), None),
             "forced": ("ASKAP", np.linspace(0.8e8, 1.2e8, 5), "LOW")}
    for k, (name, freq, array) in cases.items():
        gt = table(np.ones((2, 3, len(freq), 2, 2), complex), freq, "B", name=name)
        out[f"{k}_name"] = np.array(name)
        out[f"{k}_array"] = np.array(array or "")
        out[f"{k}_in"] = freq
        out[f"{k}_out"] = np.asarray(ref["set_beamformer_frequencies"](gt, array=array))
    assert np.all(out["low_out"] % 781.25e3 == 0)
    assert np.all(np.abs(np.diff(out["mid_out"]) - 300.0e6 / 4096) < 1e-9)
    assert np.array_equal(out["unknown_out"], out["unknown_in"])
    save("beamformer_frequencies.npz", **out)


def spectra(rng, nt, na, freq, nrec):
    """Amplitude 1 +- 0.1, a linear phase ramp plus 0.05 rad of noise, every
    (time, antenna, receptor) element its own."""
    shape = (nt, na, len(freq), nrec, nrec)
    x = ((freq - freq[0]) / (freq[-1] - freq[0]))[None, None, :, None, None]
    lead = (nt, na, 1, nrec, nrec)
    amp = 1.0 + 0.08 * rng.uniform(-1, 1, lead) * np.cos(2.0 * x + rng.uniform(0, 6, lead)) \
        + 0.02 * rng.uniform(-1, 1, shape)
    phase = rng.uniform(-np.pi, np.pi, lead) + rng.uniform(-3, 3, lead) * x \
        + 0.05 * rng.normal(size=shape)
    return amp * np.exp(1j * phase)


def make_resample(ref):
    rng = np.random.default_rng(13)
    low = lambda f: ref["set_beamformer_frequencies"](  # noqa: E731
        table(np.ones((1, 1, len(f), 1, 1), complex), f, "B"), array="LOW")
    mid = lambda f: ref["set_beamformer_frequencies"](  # noqa: E731
        table(np.ones((1, 1, len(f), 1, 1), complex), f, "B"), array="MID")
    wide_f = np.linspace(100e6, 160e6, 96)
    wide_g = spectra(rng, 2, 3, wide_f, 2)
    narrow_f = np.linspace(100e6, 105e6, 64)
    mid_f = 1.0e9 + 7.0e3 * np.arange(100)
    low_f = np.linspace(50e6, 350e6, 1536)
    d_wide = wide_f[1] - wide_f[0]
    algs3 = ("polyfit", "cubicspl", "interp")
    # name: (freq_in, gain, freq_out, edges, polydeg, algorithms)
    cases = {
        "wide": (wide_f, wide_g, low(wide_f), None, 3, algs3),
        "narrow": (narrow_f, spectra(rng, 1, 2, narrow_f, 2),
                   np.linspace(narrow_f[0], narrow_f[-1], 41)[:-1] + 3.1e4, None, 3, algs3),
        "mid": (mid_f, spectra(rng, 2, 2, mid_f, 1), mid(mid_f), None, 3, algs3),
        "deg5": (wide_f, wide_g, low(wide_f), None, 5, ("polyfit",)),
        "edges": (wide_f, wide_g, wide_f[0] + d_wide * (np.arange(-3, 99) + 0.25), [0, 30, 61], 2,
                  ("polyfit",)),
        "lowband": (low_f, spectra(rng, 1, 1, low_f, 2), low(low_f), None, None, algs3),
    }
    warnings.simplefilter("error", np.exceptions.RankWarning)
    for k, (f_in, gain, f_out, edges, deg, algs) in cases.items():
        eff = 3 if deg is None else deg
        for ratio, rcond in br.reference_condition(f_in, edges, eff):
            print(f"{k}: smallest/largest singular value {ratio:.2e}, rcond {rcond:.2e}")
            assert ratio >= 10 * rcond, (k, ratio, rcond)
        gt = table(gain, f_in, "B")
        out = dict(frequency=f_in, gain=gain, frequency_out=f_out,
                   edges=np.array([] if edges is None else edges, dtype=np.int64),
                   polydeg=np.array(-1 if deg is None else deg), algs=np.array(",".join(algs)))
        for alg in algs:
            kw = dict(edges=edges, polydeg=deg) if alg == "polyfit" else {}
            out[f"out_{alg}"] = ref["resample_bandpass"](f_out, gt, alg=alg, **kw)
        m, seg = br.tight_operator(f_out, f_in, edges, eff)
        tight = br.apply_operator(m, gain, seg)
        inside = seg >= 0
        s_case = np.max(np.abs(out["out_polyfit"][:, :, inside] - tight[:, :, inside]))
        print(f"{k}: S = max |reference - tight| = {s_case:.2e}, {np.sum(~inside)} outside")
        if k == "edges":
            assert np.array_equal(np.nonzero(~inside)[0], [0, 1, 2, 99, 100, 101])
            out["out_polyfit"][:, :, ~inside] = 0      # numpy.empty's garbage is not compared
        else:
            assert inside.all()
        out["s_polyfit"] = np.array(s_case)
        out["outside"] = ~inside
        save(f"beamformer_resample_{k}.npz", **out)


if __name__ == "__main__":
    R = reference()
    make_expand(R)
    make_multiply(R)
    make_frequencies(R)
    make_resample(R)
