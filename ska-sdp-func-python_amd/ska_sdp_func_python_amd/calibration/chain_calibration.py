"""Chains of gain tables (T, G, B) on MI355X (reference
``src/ska_sdp_func_python/calibration/chain_calibration.py``):

* ``create_calibration_controls`` (:27-72): the default controls of T, G, B.
* ``calibrate_chain`` (:137-222): per context letter solve, then take the
  solution off the visibilities (``apply_gaintable(..., inverse=True)``) before
  the next letter is solved.  The input Visibility is corrected in place.
* ``solve_calibrate_chain`` (:225-320): every letter solved against the same
  uncorrected visibilities, nothing applied.
* ``apply_calibration_chain`` (:75-134): the tables applied one after another.
  The reference does that with one ``apply_gaintable`` per table, each a full
  pass over vis and weight; here the tables go through
  ``kernels.apply_gain_chain`` (sdp_hip_apply_gain_chain), one pass in which
  an element stays in registers, with the bits of the sequential calls.  When
  a visibility time lies in more than one row's window of some table, the
  sequential ``apply_gaintable`` calls are used (they apply such rows one
  after another).

A Visibility that holds device tensors stays on the device; only the gain
tables cross.  The functions call the module-level names ``solve_gaintable``,
``apply_gaintable`` and ``create_gaintable_from_visibility``.

Two deviations from the reference, both in ``apply_calibration_chain``:

* a dict of tables is applied in the order of ``calibration_context``, for
  the letters it holds.  The reference fills its list of contexts only from
  a list of tables, so for a dict it returns the visibilities unchanged.
* ``inverse`` (default False, the reference's forward apply) is a keyword
  beyond the reference's: with it the chain ``calibrate_chain`` returned can
  be taken off another Visibility.
"""

import logging

import numpy as np
import torch

from .. import _device, kernels
from ..datamodels import GainTable, create_gaintable_from_visibility
from .operations import _store, _time_rows, apply_gaintable
from .solvers import solve_gaintable

log = logging.getLogger("func-python-logger")


def create_calibration_controls():
    """The controls of T (atmospheric phase), G (electronic gain) and B
    (bandpass); adjust the returned dictionary as needed."""
    def entry(shape, timeslice, phase_only):
        return {"shape": shape, "timeslice": timeslice, "phase_only": phase_only,
                "first_selfcal": 0}

    return {"T": entry("scalar", "auto", True), "G": entry("vector", 60.0, False),
            "B": entry("vector", 1e5, False)}


def _existing_tables(gaintables, calibration_context):
    """{jones letter: table} of a GainTable, a list (tables whose jones_type
    is in the context; a later one replaces an earlier one of its type) or a
    dict (taken as it is); anything else: no tables."""
    if isinstance(gaintables, GainTable):
        gaintables = [gaintables]
    if isinstance(gaintables, list):
        return {g.attrs["jones_type"]: g for g in gaintables
                if g.attrs["jones_type"] in list(calibration_context)}
    if isinstance(gaintables, dict):
        return gaintables
    return {}


def _solve(vis, model_vis, gain_table, control, tol):
    return solve_gaintable(vis, model_vis, gain_table=gain_table,
                           phase_only=control["phase_only"],
                           crosspol=control["shape"] == "matrix",
                           timeslice=control["timeslice"], tol=tol)


def _absmax(a):
    """max |a| (a device reduction for a device tensor)."""
    a = getattr(a, "data", a)
    if isinstance(a, torch.Tensor):
        return float(a.abs().max())
    return float(np.max(np.abs(a)))


def calibrate_chain(vis, model_vis, gaintables=None, calibration_context="T", controls=None,
                    iteration=0, tol=1e-6):
    """Solve the context's letters in order, correcting ``vis`` (in place)
    with each solution before the next; returns (vis, {letter: GainTable})."""
    if controls is None:
        controls = create_calibration_controls()
    avis = vis
    gt = _existing_tables(gaintables, calibration_context)
    for c in list(calibration_context):
        log.debug("calibrate_chain: Jones matrix %s, iteration %s", c, iteration)
        if iteration < controls[c]["first_selfcal"]:
            continue
        if c not in gt:
            log.info("Creating new %s gaintable", c)
            gt[c] = create_gaintable_from_visibility(avis, timeslice=controls[c]["timeslice"],
                                                     jones_type=c)
        gt[c] = _solve(avis, model_vis, gt[c], controls[c], tol)
        if log.isEnabledFor(logging.DEBUG):
            log.debug(gt[c].gaintable_acc.qa_gain_table(
                context=f"Jones matrix {c}, iteration {iteration}"))
        avis = apply_gaintable(avis, gt[c], inverse=True)
    return avis, gt


def solve_calibrate_chain(vis, model_vis, gaintables=None, calibration_context="T", controls=None,
                          iteration=0, tol=1e-6):
    """Solve every letter of the context against the same visibilities;
    returns {letter: GainTable}.  A letter is solved only when some flagged
    weight and (if there is a model) some model visibility is non-zero."""
    if controls is None:
        controls = create_calibration_controls()
    gt = _existing_tables(gaintables, calibration_context)
    for c in list(calibration_context):
        if c not in gt:
            gt[c] = create_gaintable_from_visibility(vis, timeslice=controls[c]["timeslice"],
                                                     jones_type=c)
        fmin, fmax = gt[c].frequency.data[0], gt[c].frequency.data[-1]
        if iteration < controls[c]["first_selfcal"]:
            log.info("Not solving for Jones matrix %s this iteration: iteration %s, "
                     "frequency %4g - %4g Hz", c, iteration, fmin, fmax)
        elif _absmax(vis.visibility_acc.flagged_weight) > 0.0 and (
                model_vis is None or _absmax(model_vis.vis) > 0.0):
            gt[c] = _solve(vis, model_vis, gt[c], controls[c], tol)
            if log.isEnabledFor(logging.INFO):
                log.info("calibrate_chain: %s", gt[c].gaintable_acc.qa_gain_table(
                    context=f"Model is non-zero: solving for Jones matrix {c}, iteration "
                            f"{iteration}, frequency {fmin:4g} - {fmax:4g} Hz"))
        else:
            log.info("No model data: cannot solve for Jones matrix %s, iteration %s, "
                     "frequency %4g - %4g Hz", c, iteration, fmin, fmax)
    return gt


def _apply_chain(vis, tables, inverse):
    """``tables`` on ``vis`` in order, in place: one pass of
    kernels.apply_gain_chain, or sequential apply_gaintable calls where a
    table's row windows overlap (or the tables differ in their antennas)."""
    vis_time = np.asarray(vis.time.data, dtype=float)
    maps = []
    for t in tables:
        rows = _time_rows(vis_time, np.asarray(t.time.data, dtype=float),
                          np.asarray(t.interval.data, dtype=float))
        tr = np.full(len(vis_time), -1, dtype=np.int32)
        hits = np.zeros(len(vis_time), dtype=int)
        for r, idx in enumerate(rows):
            tr[idx] = r
            hits[idx] += 1
        if np.any(hits > 1) or t.gaintable_acc.nants != tables[0].gaintable_acc.nants:
            for table in tables:
                vis = apply_gaintable(vis, table, inverse=inverse)
            return vis
        maps.append(tr)
    dev = _device.device()
    v = _device.to_dev(vis["vis"].data, None, dev)
    if v.dtype not in (torch.complex64, torch.complex128):
        v = v.to(torch.complex128)
    v = v.contiguous()
    w = _device.to_dev(vis["weight"].data, torch.float64, dev).contiguous()
    bl = np.asarray(vis.baselines.data)
    a1 = torch.as_tensor(bl[:, 0].astype(np.int32), device=dev)
    a2 = torch.as_tensor(bl[:, 1].astype(np.int32), device=dev)
    gains = [_device.to_dev(t["gain"].data, torch.complex128, dev).contiguous() for t in tables]
    kernels.apply_gain_chain(v, w, a1, a2, [torch.as_tensor(m, device=dev) for m in maps], gains,
                             inverse)
    _store(vis, "vis", v)
    _store(vis, "weight", w)
    return vis


def apply_calibration_chain(vis, gaintables, calibration_context="T", controls=None, iteration=0,
                            inverse=False):
    """Apply (``inverse``: take off) the tables whose letter is in the context
    and whose ``first_selfcal`` the iteration has reached: a list in list
    order, a dict in context order.  ``vis`` is changed in place and returned."""
    if controls is None:
        controls = create_calibration_controls()
    if isinstance(gaintables, GainTable):
        gaintables = [gaintables]
    if isinstance(gaintables, list):
        # as the reference: one entry per listed table, each entry looked up by
        # its letter (a letter listed twice applies its last table twice)
        gt = _existing_tables(gaintables, calibration_context)
        contexts = [g.attrs["jones_type"] for g in gaintables if g.attrs["jones_type"] in gt]
    elif isinstance(gaintables, dict):
        gt = gaintables
        contexts = [c for c in list(calibration_context) if c in gt]
    else:
        log.warning("Invalid GainTable format supplied. Visibility not updated.")
        return vis
    tables = [gt[c] for c in contexts if iteration >= controls[c]["first_selfcal"]]
    if tables:
        vis = _apply_chain(vis, tables, inverse)
    return vis
