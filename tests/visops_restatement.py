"""Plain-numpy restatements of the reference's visibility operations
(src/ska_sdp_func_python/visibility/operations.py) on bare arrays
[ntimes, nbl, nchan, npol], pinned to the reference's outputs in
tests/golden/visops_*.npz by tests/test_visops_cpu.py and used as the
reference at the shapes the GPU tests choose.  The sums are numpy.sum(axis=-2)
itself, so their order of addition is numpy's; the polynomial fit is a QR
solve of the weighted, column-scaled Vandermonde matrix."""

import warnings

import numpy as np

from conftest import golden


def integrate(vis, weight, iw, flags):
    """integrate_visibility_by_channel (:192-235): (vis, weight, imaging_weight,
    flags), each [nt, nbl, 1, npol]."""
    nchan = vis.shape[2]
    keep = 1 - flags
    fw = weight * keep
    fl = np.sum(flags, axis=-2)[..., np.newaxis, :]
    fl[fl < nchan] = 0
    fl[fl > 1] = 1
    newvis = np.sum(vis * fw, axis=-2)[..., np.newaxis, :]
    neww = np.sum(fw, axis=-2)[..., np.newaxis, :]
    newiw = np.sum(iw * keep, axis=-2)[..., np.newaxis, :]
    d = (1 - fl) * neww
    mask = d > 0.0
    newvis[mask] = newvis[mask] / d[mask]
    return newvis, neww, newiw, fl


def average(vis, weight, iw, flags, G):
    """average_visibility_by_channel (:238-306), the list stacked along the
    channel axis: each [nt, nbl, nchan / G, npol]."""
    nchan = vis.shape[2]
    keep = 1 - flags
    outs = ([], [], [], [])
    for g0 in range(0, nchan, G):
        s = slice(g0, g0 + G)
        fl = np.sum(flags[..., s, :], axis=-2)[..., np.newaxis, :]
        fl[fl < nchan] = 0
        fl[fl > 1] = 1
        nv = np.sum((vis * keep)[..., s, :] * weight[..., s, :], axis=-2)[..., np.newaxis, :]
        nw = np.sum((weight * keep)[..., s, :], axis=-2)[..., np.newaxis, :]
        niw = np.sum((iw * keep)[..., s, :], axis=-2)[..., np.newaxis, :]
        d = nw * (1 - fl)
        mask = d > 0.0
        nv[mask] = nv[mask] / d[mask]
        for lst, a in zip(outs, (nv, nw, niw, fl)):
            lst.append(a)
    return tuple(np.concatenate(lst, axis=2) for lst in outs)


def to_stokes(vis, flags, frame):
    """convert_visibility_to_stokes (:309-333) of linear / circular data:
    (vis, flags)."""
    from ska_sdp_func_python_amd import datamodels as dm
    m = dm.pol_conversion_matrix(dm.PolarisationFrame(frame), dm.PolarisationFrame("stokesIQUV"))
    out = np.einsum("oi,...i->...o", m, vis)
    fl = np.logical_or(flags[..., 0], flags[..., 3])[..., np.newaxis]
    return out, np.repeat(fl.astype(flags.dtype), 4, axis=-1)


def to_stokesI(vis, weight, iw, flags):
    """convert_visibility_to_stokesI (:336-420) with the half-sum of the two
    parallel hands: (vis, weight, imaging_weight, flags), each [..., 1]."""
    keep = 1 - flags
    fv, fw, fiw = vis * keep, weight * keep, iw * keep
    nv = 0.5 * (fv[..., 0] + fv[..., -1])[..., np.newaxis]
    nw = (fw[..., 0] + fw[..., -1])[..., np.newaxis]
    niw = (fiw[..., 0] + fiw[..., -1])[..., np.newaxis]
    fl = np.logical_or(flags[..., 0], flags[..., -1])[..., np.newaxis]
    return nv, nw, niw, fl.astype(flags.dtype)


def stokesI_to_polframe(vis, weight, iw, flags, npol):
    """convert_visibility_stokesI_to_polframe (:423-471)."""
    keep = 1 - flags
    nv = np.repeat((vis * keep)[..., 0:1], npol, axis=-1)
    nv[..., 1] = 0.0
    nv[..., 2] = 0.0
    return (nv, np.repeat((weight * keep)[..., 0:1], npol, axis=-1),
            np.repeat((iw * keep)[..., 0:1], npol, axis=-1), np.repeat(flags[..., 0:1], npol, axis=-1))


def abscissa(frequency):
    f = np.asarray(frequency, dtype=float)
    n = len(f)
    return (f - f[n // 2]) / (f[0] - f[n // 2])


def fit_weights(weight, flags, mask=None):
    """The fit weight per sample: flagged_weight, 0 where mask is True (:132-136)."""
    fw = weight * (1 - flags)
    if mask is not None:
        fw = fw.copy()
        fw[:, :, np.asarray(mask, dtype=bool), :] = 0.0
    return fw


def remove_continuum(vis, weight, flags, frequency, degree, mask=None, host_route=True, x=None):
    """remove_continuum_visibility (:108-142): the visibilities with the fitted
    polynomial subtracted (complex128), and n_live per spectrum [nt, nbl, npol].
    Spectra with n_live >= degree + 1 are solved by QR; those with
    1 <= n_live <= degree by numpy.polyfit when ``host_route``, else left
    unchanged; those with n_live == 0 are left unchanged.  ``x`` replaces the
    abscissa of ``frequency``."""
    x = abscissa(frequency) if x is None else np.asarray(x, dtype=float)
    nt, nbl, nchan, npol = vis.shape
    fw = fit_weights(weight, flags, mask)
    out = np.array(vis, dtype=np.complex128)
    y = np.moveaxis(out, 2, 3).reshape(-1, nchan)          # [spectrum, chan]
    w2 = np.moveaxis(fw, 2, 3).reshape(-1, nchan)
    live = (w2 != 0).sum(axis=1)
    full = live >= degree + 1
    van = np.vander(x, degree + 1)                          # decreasing powers
    if np.any(full):
        sw = np.sqrt(w2[full])
        lhs = van[np.newaxis] * sw[:, :, np.newaxis]
        scale = np.sqrt((lhs * lhs).sum(axis=1))
        lhs = lhs / scale[:, np.newaxis, :]
        q, r = np.linalg.qr(lhs)
        qtb = np.einsum("sck,sc->sk", q, y[full] * sw)
        coef = np.linalg.solve(r.astype(complex), qtb[..., np.newaxis])[..., 0] / scale
        y[full] = y[full] - np.einsum("ck,sk->sc", van, coef)
    if host_route:
        for s in np.flatnonzero((live >= 1) & ~full):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fit = np.polyfit(x, y[s], w=np.sqrt(w2[s]), deg=degree)
            y[s] = y[s] - np.polyval(fit, x)
    out = np.moveaxis(y.reshape(nt, nbl, npol, nchan), 3, 2)
    return np.ascontiguousarray(out), live.reshape(nt, nbl, npol)


def random_case(nt, nbl, nchan, npol, seed, flag_fraction=0.15):
    """Random complex visibilities exactly representable in complex64, weights
    and imaging weights uniform(0.5, 2), ``flag_fraction`` flagged."""
    rng = np.random.default_rng(seed)
    shape = (nt, nbl, nchan, npol)
    vis = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    weight = rng.uniform(0.5, 2.0, shape)
    iw = rng.uniform(0.5, 2.0, shape)
    flags = (rng.uniform(size=shape) < flag_fraction).astype(np.int64)
    return vis.astype(np.complex128), weight, iw, flags


def case_visibility(g, to=None):
    """The Visibility of a visops golden fixture's inputs; ``to`` maps each
    data array (e.g. onto the device)."""
    from ska_sdp_func_python_amd import datamodels as dm
    to = to or (lambda a: a.copy())
    return dm.Visibility.constructor(
        frequency=g["frequency"], channel_bandwidth=g["channel_bandwidth"],
        phasecentre=dm.SkyCoord(0.0, -0.5), configuration="LOW", uvw=g["uvw"].copy(),
        time=g["time"], integration_time=g["integration_time"], vis=to(g["vis"]),
        weight=to(g["weight"]), imaging_weight=to(g["imaging_weight"]), flags=to(g["flags"]),
        baselines=g["baselines"], polarisation_frame=dm.PolarisationFrame(str(g["frame"])))


def load(name):
    return golden(f"visops_{name}.npz")
