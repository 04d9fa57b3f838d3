"""Plain numpy restatement of the complex Hogbom minor cycle (Q + iU cleaned
as one complex image), the CPU yardstick of csrc/clean.hip's complex kernel
pair: tests/test_hogbom_complex_cpu.py pins it to the reference's goldens bit
for bit, tests/test_gpu_hogbom_complex.py compares the device against it.
Unlike the reference's function it takes one PSF and also returns the cycle
count.

It is written on two real planes, one IEEE operation per step, as the kernels
are:
  * the search key of a pixel is hypot(q * w, u * w) (w = 1 without a window),
    the peak numpy.argmax of it: first maximum, row-major;
  * rinv = 1 / pmax once; mval_q = (q[peak] * gain) * rinv, the same for u --
    numpy's division of a complex scalar by a real one, not (q * gain) / pmax;
  * comps_q[peak] += mval_q, comps_u[peak] += mval_u;
  * on the patch of clean_restatement.patch, q -= psf * mval_q and
    u -= psf * mval_u;
  * stop once hypot(q[peak], u[peak]) < absthresh after the subtraction --
    absthresh = max(thresh, fracthresh * max hypot(q, u)) itself, without the
    0.9 of the real Hogbom; that cycle counts.

numpy's complex absolute is not hypot bit for bit; the goldens keep every
decision (peak, stop) at least 1e-9 away from a tie, so the two agree on them.
A NaN key is not handled here: numpy.argmax would select it, the device never
does.
"""

import numpy as np

from clean_restatement import patch


def cases():
    """The golden cases' names."""
    return [f"C{i}" for i in range(1, 12)]


def load_case(name, golden):
    """Inputs, settings and expected outputs of golden case ``name``;
    ``golden`` is conftest.golden."""
    inp = golden("clean_inputs.npz")
    inp_u = golden("hogbom_complex_inputs.npz")
    g = golden(f"hogbom_complex_{name}.npz")
    dk, wk = str(g["dirty_key"]), str(g["window_key"])
    return dict(dirty_q=inp[dk], dirty_u=inp_u[dk + "_u"],
                psf=float(g["psf_scale"]) * inp[str(g["psf_key"])],
                window=inp[wk] if wk else None, gain=float(g["gain"]), thresh=float(g["thresh"]),
                niter=int(g["niter"]), fracthresh=float(g["fracthresh"]), cycles=int(g["cycles"]),
                min_gap=float(g["min_gap"]),
                expect=tuple(g[k] for k in ("comps_q", "comps_u", "res_q", "res_u")))


def hogbom_complex(dirty_q, dirty_u, psf, window, gain, thresh, niter, fracthresh):
    """-> comps_q, comps_u, res_q, res_u, cycles"""
    q, u = np.array(dirty_q, dtype=float), np.array(dirty_u, dtype=float)
    absthresh = max(thresh, fracthresh * np.hypot(q, u).max())
    comps_q, comps_u = np.zeros(q.shape), np.zeros(q.shape)
    rinv = 1.0 / psf.max()
    it = 0
    for i in range(niter):
        it = i + 1
        key = np.hypot(q, u) if window is None else np.hypot(q * window, u * window)
        py, px = np.unravel_index(key.argmax(), q.shape)
        mval_q = (q[py, px] * gain) * rinv
        mval_u = (u[py, px] * gain) * rinv
        comps_q[py, px] += mval_q
        comps_u[py, px] += mval_u
        img, box = patch(q.shape, psf.shape, py, px)
        q[img] -= psf[box] * mval_q
        u[img] -= psf[box] * mval_u
        if np.hypot(q[py, px], u[py, px]) < absthresh:
            break
    return comps_q, comps_u, q, u, it
