"""Plain numpy restatement of the multi-scale multi-frequency CLEAN minor
cycle (Rau & Cornwell 2011, Algorithm 1), the CPU yardstick of
csrc/mfsclean.hip: tests/test_mfsclean_cpu.py pins it to the reference's
goldens bit for bit, tests/test_gpu_mfsclean.py compares the device against
it.  Every sum is an explicit left-to-right loop (no einsum), and it also
returns the iteration count and the cycles that chose each scale.

State: r[s, t] the residual moments smoothed by scale s; P[a, b, k] the PSF
moment k smoothed by scales a and b (k = t + q stands for every moment pair);
hs[s][t, q] = P[s, s, t + q] at the PSF origin, ihs[s] its inverse.

One cycle:
  * sol[s, n] = ((ihs[s][0, n] * r[s, 0]) + ihs[s][1, n] * r[s, 1]) + ...
  * the search field of scale s is sol[s, 0]; for findpeak "CASA" it is
    d = 0; for m1: d += (2 * sol[s, m1]) * r[s, m1];
               for m2: d -= (hs[s][m1, m2] * sol[s, m1]) * sol[s, m2]
  * per scale the pixel is argmax |field[s]| (first maximum, row-major),
    WITHOUT window or sensitivity; the scales are compared on
    max |field[s] * window[s] * sensitivity| with a strict '>' from 0, so
    that the window and the sensitivity choose the scale, not the pixel;
    nothing above 0 leaves pixel (0, 0) of scale 0;
  * mval[n] = sol[scale, n, pixel]; the cycle and its scale are counted;
    stop if |mval[0]| < absthresh (before the update);
  * over the patch [peak - p // 2, peak + p // 2) clipped, PSF pixel p // 2
    on the peak:
      r[s, t] -= gain * (((P[scale, s, t] * mval[0]) + P[scale, s, t + 1] * mval[1]) + ...)
      model[t] += (scale kernel * gain) * mval[t]

The set-up (scale kernels, FFT convolutions) is the package's host code;
``fft="torch"`` runs it with torch.fft on CPU tensors instead of numpy.fft --
the one difference between the host and the device set-up.
"""

import numpy as np
import torch

from clean_restatement import patch
from ska_sdp_func_python_amd.image import cleaners


def setup(dirty, psf, window, scales, fft="numpy"):
    """-> r [S, T, ny, nx], P [S, S, 2T - 1, py, px], scale kernels (PSF-sized),
    hs, ihs [S, T, T], window stack or None, pmax"""
    pmax = psf.max()
    lpsf, ldirty = psf / pmax, dirty / pmax
    nt = dirty.shape[0]
    assert nt == 1 or psf.shape[0] == 2 * nt
    ns = len(scales)
    stack = cleaners.create_scalestack([ns, *ldirty.shape[1:]], scales, norm=True)
    pstack = cleaners.create_scalestack([ns, *lpsf.shape[1:]], scales, norm=True)
    if fft == "torch":
        t = torch.as_tensor
        conv = lambda s, img: cleaners.convolve_scalestack(t(s), t(img)).numpy()
        conv2 = lambda s, img: cleaners.convolve_convolve_scalestack(t(s), t(img)).numpy()
    else:
        conv, conv2 = cleaners.convolve_scalestack, cleaners.convolve_convolve_scalestack
    r = np.zeros((ns, nt) + ldirty.shape[1:])
    for m in range(nt):
        r[:, m] = conv(stack, ldirty[m])
    P = np.zeros((ns, ns, 2 * nt - 1) + lpsf.shape[1:])
    for k in range(2 * nt - 1):
        P[:, :, k] = conv2(pstack, lpsf[k])
    cy, cx = lpsf.shape[1] // 2, lpsf.shape[2] // 2
    hs = np.zeros((ns, nt, nt))
    ihs = np.zeros((ns, nt, nt))
    for s in range(ns):
        for a in range(nt):
            for b in range(nt):
                hs[s, a, b] = P[s, s, a + b, cy, cx]
        ihs[s] = np.linalg.inv(hs[s])
    wstack = None
    if window is not None:
        wstack = np.zeros_like(stack)
        wstack[conv(stack, np.asarray(window, dtype=float)) > 0.9] = 1.0
    return r, P, pstack, hs, ihs, wstack, pmax


def principal_solution(r, ihs):
    ns, nt = r.shape[:2]
    sol = np.zeros_like(r)
    for s in range(ns):
        for n in range(nt):
            acc = ihs[s, 0, n] * r[s, 0]
            for m in range(1, nt):
                acc = acc + ihs[s, m, n] * r[s, m]
            sol[s, n] = acc
    return sol


def search_field(r, sol, hs, findpeak):
    """[S, ny, nx]"""
    if findpeak != "CASA":
        return sol[:, 0]
    ns, nt = r.shape[:2]
    field = np.zeros((ns,) + r.shape[2:])
    for s in range(ns):
        for m1 in range(nt):
            field[s] = field[s] + (2.0 * sol[s, m1]) * r[s, m1]
            for m2 in range(nt):
                field[s] = field[s] - (hs[s, m1, m2] * sol[s, m1]) * sol[s, m2]
    return field


def find_peak(field, sens, wstack):
    """-> py, px, scale"""
    best, py, px, ps = 0.0, 0, 0, 0
    for s in range(field.shape[0]):
        weighted = field[s] if wstack is None else field[s] * wstack[s]
        if sens is not None:
            weighted = sens * weighted  # a 3-D sensitivity broadcasts: the maximum is over its moments too
        this_max = np.abs(weighted).max()
        if this_max > best:
            best, ps = this_max, s
            py, px = np.unravel_index(np.abs(field[s]).argmax(), field[s].shape)
    return int(py), int(px), ps


def minor_cycles(r, model, P, pstack, hs, ihs, wstack, sens, gain, absthresh, niter, findpeak):
    """Up to ``niter`` cycles in place on ``r`` and ``model`` -> iterations, cycles per scale"""
    ns, nt = r.shape[:2]
    counts = [0] * ns
    it = 0
    for i in range(niter):
        it = i + 1
        sol = principal_solution(r, ihs)
        py, px, ps = find_peak(search_field(r, sol, hs, findpeak), sens, wstack)
        mval = sol[ps, :, py, px]
        counts[ps] += 1
        if np.abs(mval[0]) < absthresh:
            break
        img, box = patch(r.shape[2:], P.shape[3:], py, px)
        for t in range(nt):
            model[t][img] += (pstack[ps][box] * gain) * mval[t]
        for s in range(ns):
            for t in range(nt):
                acc = P[ps, s, t][box] * mval[0]
                for q in range(1, nt):
                    acc = acc + P[ps, s, t + q][box] * mval[q]
                r[s, t][img] -= gain * acc
    return it, counts


def msmfsclean(dirty, psf, window, sens, gain, thresh, niter, scales, fracthresh,
               findpeak="RASCIL", fft="numpy"):
    """-> model [T, ny, nx], residual [T, ny, nx], iterations, cycles per scale"""
    r, P, pstack, hs, ihs, wstack, pmax = setup(dirty, psf, window, scales, fft)
    absthresh = max(thresh, fracthresh * np.abs(r[0, 0]).max())
    model = np.zeros(dirty.shape)
    it, counts = minor_cycles(r, model, P, pstack, hs, ihs, wstack, sens, gain, absthresh, niter,
                              findpeak)
    return model, pmax * r[0], it, counts
