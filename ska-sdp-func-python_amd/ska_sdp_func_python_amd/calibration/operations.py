"""apply_gaintable on MI355X (reference
``src/ska_sdp_func_python/calibration/operations.py:23-256``).

The reference's per gain row x vis row x baseline x channel Python loop
becomes one HIP kernel over (time, baseline, channel) (sdp_hip_apply_gains)
plus a small kernel forming the effective gains (the scalar reciprocal or
the 2x2 inverse with the singular-gain test).  The vis rows a gain row owns
are ``|t - T_r| < interval_r / 2`` (strict, operations.py:57-61).  When a
vis time falls in more than one gain row's window the reference applies
the rows one after another; so does this, one launch per gain row.  The
input Visibility is modified in place and returned, as in the reference.

``multiply_gaintables`` (:259-299) and ``concatenate_gaintables`` (:302-320)
work on the gain tables alone (O(gain table): numpy for host arrays, torch
for device tensors, no kernel).  The 2x2 product is the reference's
``einsum("...ik,...ij->...kj")``, the transpose of ``gt`` times ``dgt`` per
matrix, kept as the reference computes it.
"""

import logging

import numpy as np
import torch

from .. import _device, kernels
from ..datamodels import GainTable

log = logging.getLogger("func-python-logger")


def _time_rows(vis_time, gt_time, interval):
    """[nrow_g][vis time indices] with the reference's strict window."""
    return [np.nonzero(np.abs(vis_time - gt_time[r]) < interval[r] / 2.0)[0]
            for r in range(len(gt_time))]


def _store(vis, name, value):
    cur = vis[name].data
    if _device.is_device(cur):
        if cur.data_ptr() != value.data_ptr():
            cur.copy_(value.reshape(cur.shape))
    else:
        cur[...] = value.reshape(cur.shape).cpu().numpy()


def apply_gaintable(vis, gt, inverse=False, use_flags=False):
    ntimes, nants, nchan, _, _ = gt.gain.shape
    if inverse:
        log.debug("apply_gaintable: Apply inverse gaintable")
    else:
        log.debug("apply_gaintable: Apply gaintable")
    if vis.visibility_acc.npol == 1:
        log.debug("apply_gaintable: scalar gains")
    dev = _device.device()
    vis_time = np.asarray(vis.time.data, dtype=float)
    rows = _time_rows(vis_time, np.asarray(gt.time.data, dtype=float),
                      np.asarray(gt.interval.data, dtype=float))
    nvt = len(vis_time)
    hits = np.zeros(nvt, dtype=int)
    for r in rows:
        hits[r] += 1
    if np.any(hits > 1):
        passes = [[r] for r in range(len(rows)) if len(rows[r])]  # sequential, as the reference
    else:
        passes = [list(range(len(rows)))]
    v = _device.to_dev(vis["vis"].data, None, dev)
    if v.dtype not in (torch.complex64, torch.complex128):
        v = v.to(torch.complex128)
    v = v.contiguous()
    w = _device.to_dev(vis["weight"].data, torch.float64, dev).contiguous()
    fl = None
    if use_flags:
        fl = _device.to_dev(vis["flags"].data, None, dev)
        if fl.dtype not in kernels.FLAG_BYTES:
            fl = fl.to(torch.int64)
        fl = fl.contiguous()
    bl = np.asarray(vis.baselines.data)
    a1 = torch.as_tensor(bl[:, 0].astype(np.int32), device=dev)
    a2 = torch.as_tensor(bl[:, 1].astype(np.int32), device=dev)
    gain = _device.to_dev(gt["gain"].data, torch.complex128, dev).contiguous()
    for rs in passes:
        tr = np.full(nvt, -1, dtype=np.int32)
        for r in rs:
            tr[rows[r]] = r
        if not np.any(tr >= 0):
            continue
        kernels.apply_gains(v, w, fl, use_flags, a1, a2, torch.as_tensor(tr, device=dev), gain,
                            inverse)
    _store(vis, "vis", v)
    _store(vis, "weight", w)
    return vis


def _is_tensor(a):
    return isinstance(a, torch.Tensor)


def multiply_gaintables(gt, dgt, time_tolerance=1e-3):
    """gt * dgt, written into ``gt`` and returned (operations.py:259-299)."""
    mismatch = np.max(np.abs(np.asarray(gt["time"].data, dtype=float)
                             - np.asarray(dgt["time"].data, dtype=float)))
    if mismatch > time_tolerance:
        raise ValueError(f"Gaintables not aligned in time: max mismatch {mismatch} seconds")
    nrec = dgt.gaintable_acc.nrec
    if nrec != gt.gaintable_acc.nrec:
        raise ValueError(f"Gain tables have different structures {str(gt)} {str(dgt)}")
    if nrec not in (1, 2):
        raise ValueError(f"Gain tables have illegal structures {str(gt)} {str(dgt)}")
    a, b = gt["gain"].data, dgt["gain"].data
    wa, wb = gt["weight"].data, dgt["weight"].data
    if _is_tensor(a) or _is_tensor(b):
        a = _device.to_dev(a, None, b.device if _is_tensor(b) else a.device)
        b = _device.to_dev(b, a.dtype, a.device)
        wb = _device.to_dev(wb, None, a.device)
        wa = _device.to_dev(wa, wb.dtype, a.device)
        ein = torch.einsum
    else:
        ein = np.einsum
    gt["gain"].data = ein("...ik,...ij->...kj", a, b) if nrec == 2 else a * b
    gt["weight"].data = wa * wb
    return gt


def _cat(arrays, axis):
    if any(_is_tensor(a) for a in arrays):
        dev = next(a.device for a in arrays if _is_tensor(a))
        return torch.cat([_device.to_dev(a, None, dev) for a in arrays], dim=axis)
    return np.concatenate([np.asarray(a) for a in arrays], axis=axis)


def concatenate_gaintables(gt_list, dim="time"):
    """The tables joined along ``dim`` (operations.py:302-320: xarray.concat
    of the variables that have the dimension, everything else and the
    attributes from the first table)."""
    if len(gt_list) == 0:
        raise ValueError("GainTable list is empty")
    if dim == "time":
        axes = {"gain": 0, "weight": 0, "residual": 0, "time": 0, "interval": 0}
    elif dim == "frequency":
        axes = {"gain": 2, "weight": 2, "residual": 1, "frequency": 0}
    else:
        raise ValueError(f"concatenate_gaintables: cannot concatenate along {dim}")
    first = gt_list[0]
    v = {}
    for name in ("gain", "time", "interval", "weight", "residual", "frequency"):
        if name in axes:
            v[name] = _cat([g[name].data for g in gt_list], axes[name])
        else:
            v[name] = first[name].data
    return GainTable.constructor(v["gain"], v["time"], v["interval"], v["weight"], v["residual"],
                                 v["frequency"], first.attrs["receptor_frame"],
                                 first.attrs["phasecentre"], first.attrs["configuration"],
                                 first.attrs["jones_type"])
