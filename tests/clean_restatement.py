"""Plain numpy restatement of the Hogbom and multi-scale CLEAN minor cycles,
the CPU yardstick of the HIP kernels (tests/test_clean_cpu.py pins it to the
reference's goldens bit for bit, tests/test_gpu_clean.py compares the device
against it).  Unlike the reference's functions it also returns the iteration
count.

Semantics:
  * the peak is numpy.argmax of the search image: first maximum, row-major;
  * the patch is [peak - p // 2, peak + p // 2) clipped to the image, PSF
    pixel p // 2 on the peak (so the last row / column of an odd PSF is unused);
  * hogbom: mval = res[peak] * gain / pmax, res[patch] -= psf[patch] * mval,
    stop once |res[peak]| < 0.9 * absthresh after the subtraction;
  * msclean: per scale the search image is res * window / coupling (* sens),
    its peak found on |. * sens| and scales compared on |.| with a strict '>';
    mval = res[scale, peak] / coupling; stop before the update once
    |res[scale, peak]| < 0.9 * absthresh or mval == 0; then
    res[i, patch] -= psf[i, scale, patch] * gain * mval for every scale i and
    comps[patch] += scale kernel[patch] * gain * mval.

The msclean set-up (scale kernels, FFT convolutions) is the package's host
code, ``fft="torch"`` runs it with torch.fft on CPU tensors instead of
numpy.fft -- the one difference between the host and the device set-up.
"""

import numpy as np
import torch

from ska_sdp_func_python_amd.image import cleaners


def patch(shape, pshape, py, px):
    """(image slices, PSF slices) of the patch around peak (py, px)."""
    hy, hx = pshape[0] // 2, pshape[1] // 2
    y0, y1 = max(0, py - hy), min(shape[0], py + hy)
    x0, x1 = max(0, px - hx), min(shape[1], px + hx)
    img = (slice(y0, y1), slice(x0, x1))
    box = (slice(hy + y0 - py, hy + y1 - py), slice(hx + x0 - px, hx + x1 - px))
    return img, box


def hogbom(dirty, psf, window, gain, thresh, niter, fracthresh):
    """-> comps, residual, iterations"""
    absthresh = max(thresh, fracthresh * np.abs(dirty).max())
    comps = np.zeros(dirty.shape)
    res = np.array(dirty, dtype=float)
    pmax = psf.max()
    it = 0
    for i in range(niter):
        it = i + 1
        search = np.abs(res) if window is None else np.abs(res * window)
        py, px = np.unravel_index(search.argmax(), res.shape)
        mval = res[py, px] * gain / pmax
        comps[py, px] += mval
        img, box = patch(res.shape, psf.shape, py, px)
        res[img] -= psf[box] * mval
        if np.abs(res[py, px]) < 0.9 * absthresh:
            break
    return comps, res, it


def msclean_setup(dirty, psf, window, scales, fft="numpy"):
    """-> res stack, psf cross terms, scale kernels (PSF-sized), coupling, window stack, pmax"""
    pmax = psf.max()
    lpsf, ldirty = psf / pmax, dirty / pmax
    ns = len(scales)
    stack = cleaners.create_scalestack([ns, *ldirty.shape], scales, norm=True)
    pstack = cleaners.create_scalestack([ns, *lpsf.shape], scales, norm=True)
    if fft == "torch":
        t = torch.as_tensor
        conv = lambda s, img: cleaners.convolve_scalestack(t(s), t(img)).numpy()
        conv2 = lambda s, img: cleaners.convolve_convolve_scalestack(t(s), t(img)).numpy()
    else:
        conv, conv2 = cleaners.convolve_scalestack, cleaners.convolve_convolve_scalestack
    res = conv(stack, ldirty)
    cross = conv2(pstack, lpsf)
    coupling = np.array([[cross[i, j].max() for j in range(ns)] for i in range(ns)])
    wstack = None
    if window is not None:
        wstack = np.zeros_like(stack)
        wstack[conv(stack, np.asarray(window, dtype=float)) > 0.9] = 1.0
        assert wstack.sum() > 0
    return res, cross, pstack, coupling, wstack, pmax


def find_peak(res, sens, wstack, coupling):
    best, py, px, ps = 0.0, 0, 0, 0
    for s in range(res.shape[0]):
        resid = res[s] / coupling[s, s] if wstack is None else res[s] * wstack[s] / coupling[s, s]
        if sens is not None:
            resid = resid * sens
            y, x = np.unravel_index(np.abs(resid * sens).argmax(), resid.shape)
        else:
            y, x = np.unravel_index(np.abs(resid).argmax(), resid.shape)
        if np.abs(resid[y, x]) > best:
            best, py, px, ps = np.abs(resid[y, x]), y, x, s
    return py, px, ps


def msclean(dirty, psf, window, sens, gain, thresh, niter, scales, fracthresh, fft="numpy"):
    """-> comps, residual, iterations"""
    res, cross, pstack, coupling, wstack, pmax = msclean_setup(dirty, psf, window, scales, fft)
    absthresh = max(thresh, fracthresh * np.abs(res[0]).max())
    comps = np.zeros(dirty.shape)
    it = 0
    for i in range(niter):
        it = i + 1
        py, px, ps = find_peak(res, sens, wstack, coupling)
        mval = res[ps, py, px] / coupling[ps, ps]
        if np.abs(res[ps, py, px]) < 0.9 * absthresh:
            break
        if not np.abs(mval) > 0:
            break
        img, box = patch(dirty.shape, psf.shape, py, px)
        for s in range(len(scales)):
            res[s][img] -= cross[s, ps][box] * gain * mval
        comps[img] += pstack[ps][box] * gain * mval
    return comps, pmax * res[0], it
