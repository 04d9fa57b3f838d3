"""Generate the complex Hogbom golden fixtures tests/golden/hogbom_complex_*.npz
from the REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_hogbom_complex.py

The reference's hogbom_complex (image/cleaners.py:136-232) and overlapIndices
are AST-extracted and executed with numpy, as make_golden_clean.py does.  Only
inputs and outputs are stored -- no reference source text.

Fixtures:
  hogbom_complex_inputs.npz  the U dirty images (dirty_a_u, dirty_b_u,
                             dirty_c_u).  Q, the PSFs and the window are those
                             of clean_inputs.npz, which this generator checks
                             it reproduces
  hogbom_complex_<case>.npz  comps_q, comps_u, res_q, res_u and the settings
                             of one case (C1..C11); dirty_key, psf_key and
                             window_key name arrays of clean_inputs.npz (the U
                             image is dirty_key + "_u"), psf_scale multiplies
                             the PSF

Inputs: Q is make_golden_clean.make_inputs(seed), U make_inputs(seed + 100);
both are cleaned with Q's PSF.

Gap condition: at every cycle of every case the relative gap between the best
and the second-best |P| (times the window) is >= 1e-9, and so is the relative
distance between |P| at the peak after the subtraction and the stop threshold.
numpy's complex absolute is not hypot bit for bit, so no golden may rest on a
near-tie of either kind.  min_gap stores the smaller of the two (search_gap
and stop_margin each of them).  A seed that misses the condition is skipped
and the next one tried.
"""

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import load_reference, save  # noqa: E402
from make_golden_clean import CLEANER_DEFS, MIN_GAP, NearTie, _gap, make_inputs  # noqa: E402


class _GapArray(np.ndarray):
    """|res * window| whose argmax records the gap it was decided by."""

    gaps = None

    def argmax(self, *a, **k):
        _GapArray.gaps.append(_gap(self))
        return np.asarray(self).argmax(*a, **k)


class _NumpyWithGaps:
    """numpy, except that absolute() of an array hands out _GapArray and abs()
    of a scalar -- the stop test's |res[peak]| -- is recorded."""

    def __init__(self):
        self.peaks = []

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def absolute(x):
        return np.absolute(x).view(_GapArray)

    def abs(self, x):
        value = np.abs(x)
        if np.ndim(value) == 0:
            self.peaks.append(float(value))
        return value


def run_hogbom_complex(dirty_q, dirty_u, psf, window, gain, thresh, niter, fracthresh):
    hooked = _NumpyWithGaps()
    ns = load_reference("image/cleaners.py", CLEANER_DEFS + ["hogbom_complex"],
                        {"time": time, "numpy": hooked})
    _GapArray.gaps = []
    out = ns["hogbom_complex"](dirty_q, dirty_u, psf, psf.copy(), window, gain, thresh, niter,
                               fracthresh)
    cycles = len(_GapArray.gaps)
    assert len(hooked.peaks) == cycles
    search_gap = min(_GapArray.gaps)
    absthresh = max(thresh, fracthresh * np.absolute(dirty_q + 1j * dirty_u).max())
    stop_margin = min(abs(p - absthresh) / absthresh for p in hooked.peaks) if absthresh > 0 else np.inf
    if min(search_gap, stop_margin) < MIN_GAP:
        raise NearTie(min(search_gap, stop_margin))
    return [np.array(a) for a in out], cycles, search_gap, stop_margin


# case: (dirty, psf, psf scale, window, gain, thresh, niter, fracthresh)
CASES = {
    "C1": ("dirty_a", "psf_a", 1.0, None, 0.1, 0.0, 300, 0.05),
    "C2": ("dirty_a", "psf_a24", 1.0, None, 0.1, 0.0, 300, 0.05),
    "C3": ("dirty_b", "psf_b33", 1.0, None, 0.1, 0.0, 300, 0.05),
    "C4": ("dirty_c", "psf_c", 1.0, None, 0.1, 0.0, 300, 0.05),
    "C5": ("dirty_a", "psf_a", 1.0, "window_a", 0.1, 0.0, 300, 0.05),
    "C6": ("dirty_a", "psf_a", 1.0, None, 0.1, 0.0, 300, 0.3),     # stops on its threshold
    "C7": ("dirty_a", "psf_a", 1.0, None, 0.1, 0.0, 37, 0.05),
    "C8": ("dirty_a", "psf_a", 1.0, None, 0.1, 0.0, 1, 0.05),
    "C9": ("dirty_a", "psf_a", 1.0, None, 0.1, 0.0, 32, 0.05),     # exactly one batch of cycles
    "C10": ("dirty_b", "psf_a", 1.0, None, 0.1, 0.0, 300, 0.05),   # PSF larger than the image
    "C11": ("dirty_a", "psf_a", 0.97, None, 0.1, 0.0, 300, 0.05),  # pmax 0.97: the reciprocal rule
}


def make_cases(seed):
    inp, inp_u = make_inputs(seed), make_inputs(seed + 100)
    out = {}
    for name, (dk, pk, scale, wk, gain, thresh, niter, fracthresh) in CASES.items():
        t0 = time.time()
        (comps_q, comps_u, res_q, res_u), cycles, search_gap, stop_margin = run_hogbom_complex(
            inp[dk], inp_u[dk], scale * inp[pk], None if wk is None else inp[wk], gain, thresh,
            niter, fracthresh)
        print(f"{name}: {cycles} cycles, {np.count_nonzero(comps_q)} component pixels, search gap "
              f"{search_gap:.2e}, stop margin {stop_margin:.2e}, {time.time() - t0:.2f} s")
        out[name] = dict(comps_q=comps_q, comps_u=comps_u, res_q=res_q, res_u=res_u, dirty_key=dk,
                         psf_key=pk, psf_scale=scale, window_key=wk or "", gain=gain, thresh=thresh,
                         niter=niter, fracthresh=fracthresh, cycles=cycles, search_gap=search_gap,
                         stop_margin=stop_margin, min_gap=min(search_gap, stop_margin), seed=seed)
    return inp, inp_u, out


def make_hogbom_complex():
    for seed in range(5, 50):
        try:
            inp, inp_u, cases = make_cases(seed)
        except NearTie as e:
            print(f"seed {seed}: near-tie (gap {e.args[0]:.2e}), trying the next")
            continue
        committed = np.load(os.path.join(HERE, "clean_inputs.npz"))
        for key in {c[k] for c in CASES.values() for k in (0, 1, 3) if c[k]}:
            assert np.array_equal(inp[key], committed[key]), f"clean_inputs.npz holds another {key}"
        save("hogbom_complex_inputs.npz",
             **{f"{k}_u": inp_u[k] for k in sorted({c[0] for c in CASES.values()})})
        for name, arrays in cases.items():
            save(f"hogbom_complex_{name}.npz", **arrays)
        return
    raise RuntimeError("no seed met the gap condition")


if __name__ == "__main__":
    make_hogbom_complex()
