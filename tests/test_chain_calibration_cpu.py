"""Host logic of the calibration chain (calibration/chain_calibration.py), the
gain-table operations and apply_jones, without a GPU.

solve_gaintable / apply_gaintable (and the one-pass apply) are replaced by
recorders: what is checked is which calls the chain functions make, in which
order and with which keywords, against the reference's (chain_calibration.py
:137-320).  multiply_gaintables and apply_jones are compared with the
reference's own results (tests/golden/gaintable_ops.npz): fp64 products of two
or three factors, rtol 1e-14.
"""

import json
import logging

import numpy as np
import pytest

import chain_cases as cc
from conftest import golden

from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd.calibration import (apply_calibration_chain, apply_jones,
                                                 calibrate_chain, chain_calibration,
                                                 concatenate_gaintables,
                                                 create_calibration_controls,
                                                 multiply_gaintables, solve_calibrate_chain)


@pytest.fixture
def calls(monkeypatch):
    """Recorders in place of the solver and both apply paths."""
    log = []

    def solve(vis, modelvis=None, **kw):
        log.append(("solve", kw["gain_table"].attrs["jones_type"], vis, modelvis, kw))
        return kw["gain_table"]

    def apply(vis, gt, inverse=False, use_flags=False):
        log.append(("apply", gt.attrs["jones_type"], vis, gt, inverse))
        return vis

    def apply_chain(vis, tables, inverse):
        log.append(("chain", "".join(t.attrs["jones_type"] for t in tables), vis, tables, inverse))
        return vis

    monkeypatch.setattr(chain_calibration, "solve_gaintable", solve)
    monkeypatch.setattr(chain_calibration, "apply_gaintable", apply)
    monkeypatch.setattr(chain_calibration, "_apply_chain", apply_chain)
    return log


def _case(name):
    g = golden(f"chain_{name}.npz")
    vis, model = cc.observation(g)
    return (g, vis, model) + cc.settings(g)


def test_controls_are_the_references():
    g = golden("chain_T_p1.npz")   # stores the reference's dictionary unchanged
    assert create_calibration_controls() == json.loads(str(g["controls"]))
    a = create_calibration_controls()
    a["T"]["first_selfcal"] = 3
    assert create_calibration_controls()["T"]["first_selfcal"] == 0


def test_calibrate_chain_call_sequence(calls):
    g, vis, model, context, controls, iteration = _case("TGB_p4")
    out, gt = calibrate_chain(vis, model, calibration_context=context, controls=controls,
                              iteration=iteration, tol=3e-7)
    assert out is vis and list(gt) == ["T", "G", "B"]
    assert [(c[0], c[1]) for c in calls] == [("solve", "T"), ("apply", "T"), ("solve", "G"),
                                             ("apply", "G"), ("solve", "B"), ("apply", "B")]
    for kind, c, v, other, extra in calls:
        assert v is vis
        if kind == "solve":
            assert other is model
            assert extra == dict(gain_table=gt[c], phase_only=controls[c]["phase_only"],
                                 crosspol=False, timeslice=controls[c]["timeslice"], tol=3e-7)
        else:
            assert other is gt[c] and extra is True
    # the tables were created per context, as create_gaintable_from_visibility makes them
    assert gt["T"]["gain"].data.shape == g["cal_T_gain"].shape
    assert gt["G"]["gain"].data.shape == g["cal_G_gain"].shape
    assert gt["B"]["gain"].data.shape == g["cal_B_gain"].shape
    for c in "TGB":
        np.testing.assert_array_equal(gt[c]["time"].data, g[f"cal_{c}_time"])
        np.testing.assert_array_equal(gt[c]["interval"].data, g[f"cal_{c}_interval"])
        assert gt[c].attrs["jones_type"] == c


def test_crosspol_follows_shape(calls):
    g, vis, model, context, controls, iteration = _case("TGB_p4")
    controls["G"]["shape"] = "matrix"
    calibrate_chain(vis, model, calibration_context="TG", controls=controls)
    assert [c[4]["crosspol"] for c in calls if c[0] == "solve"] == [False, True]


def test_solve_calibrate_chain_call_sequence(calls):
    g, vis, model, context, controls, iteration = _case("TGB_p4")
    gt = solve_calibrate_chain(vis, model, calibration_context=context, controls=controls,
                               iteration=iteration)
    assert list(gt) == ["T", "G", "B"]
    assert [(c[0], c[1]) for c in calls] == [("solve", "T"), ("solve", "G"), ("solve", "B")]
    for _, c, v, m, kw in calls:
        assert v is vis and m is model
        assert kw == dict(gain_table=gt[c], phase_only=controls[c]["phase_only"], crosspol=False,
                          timeslice=controls[c]["timeslice"], tol=1e-6)


def test_first_selfcal_gate(calls):
    g, vis, model, context, controls, iteration = _case("GB_p2_gated")
    _, gt = calibrate_chain(vis, model, calibration_context=context, controls=controls,
                            iteration=iteration)
    assert list(gt) == [c for c in str(g["cal_letters"])] == ["G"]
    assert [(c[0], c[1]) for c in calls] == [("solve", "G"), ("apply", "G")]
    del calls[:]
    gt = solve_calibrate_chain(vis, model, calibration_context=context, controls=controls,
                               iteration=iteration)
    assert list(gt) == [c for c in str(g["sol_letters"])] == ["G", "B"]
    assert [(c[0], c[1]) for c in calls] == [("solve", "G")]
    np.testing.assert_array_equal(gt["B"]["gain"].data, g["sol_B_gain"])   # as created
    del calls[:]
    calibrate_chain(vis, model, calibration_context=context, controls=controls, iteration=1)
    assert [c[1] for c in calls if c[0] == "solve"] == ["G", "B"]


def test_solve_calibrate_chain_needs_weight_and_model(calls):
    g, vis, model, context, controls, iteration = _case("solve_nomodel")
    zero = vis.copy(deep=True)
    zero["weight"].data[...] = 0.0
    gt = solve_calibrate_chain(zero, model, calibration_context=context, controls=controls)
    assert not calls and list(gt) == ["T", "G"]
    for c in "TG":
        np.testing.assert_array_equal(gt[c]["gain"].data, g[f"zerowt_{c}_gain"])
        np.testing.assert_array_equal(gt[c]["weight"].data, g[f"zerowt_{c}_weight"])
    flagged = vis.copy(deep=True)
    flagged["flags"].data[...] = 1
    assert solve_calibrate_chain(flagged, model, calibration_context=context, controls=controls)
    assert not calls
    nomodel = model.copy(deep=True)
    nomodel["vis"].data[...] = 0.0
    solve_calibrate_chain(vis, nomodel, calibration_context=context, controls=controls)
    assert not calls
    solve_calibrate_chain(vis, None, calibration_context=context, controls=controls)
    assert [(c[0], c[1], c[3]) for c in calls] == [("solve", "T", None), ("solve", "G", None)]


def test_existing_tables_in_three_forms(calls):
    g, vis, model, context, controls, iteration = _case("existing")
    t_in, g_in, b_in = (cc.table(g, f"in_{c}", c, vis) for c in "TGB")
    # a single GainTable: used for its own letter, the other letter is created
    _, gt = calibrate_chain(vis, model, gaintables=t_in, calibration_context=context,
                            controls=controls)
    assert gt["T"] is t_in and list(gt) == ["T", "G"]
    assert np.all(gt["G"]["gain"].data == 1.0)
    # a list: the table of a jones_type outside the context is ignored
    del calls[:]
    _, gt = calibrate_chain(vis, model, gaintables=[g_in, t_in, b_in],
                            calibration_context=context, controls=controls)
    assert set(gt) == {"T", "G"} and gt["T"] is t_in and gt["G"] is g_in
    assert [(c[0], c[1]) for c in calls] == [("solve", "T"), ("apply", "T"), ("solve", "G"),
                                             ("apply", "G")]
    assert sorted(str(g["list_cal_letters"])) == ["G", "T"]
    # a dict: taken as it is
    given = {"T": t_in, "G": g_in}
    _, gt = calibrate_chain(vis, model, gaintables=given, calibration_context=context,
                            controls=controls)
    assert gt is given
    gt = solve_calibrate_chain(vis, model, gaintables=[b_in, g_in], calibration_context=context,
                               controls=controls)
    assert gt["G"] is g_in and set(gt) == {"T", "G"}


def test_apply_calibration_chain_order_and_gate(calls):
    g = golden("chain_apply_list.npz")
    vis, _ = cc.observation(g)
    t_in, g_in = cc.table(g, "in_T", "T", vis), cc.table(g, "in_G", "G", vis)
    foreign = cc.table(g, "in_T", "B", vis)
    assert apply_calibration_chain(vis, [g_in, foreign, t_in], calibration_context="TG") is vis
    assert calls[-1][1] == "GT" and calls[-1][4] is False     # list order, forward
    assert calls[-1][3][0] is g_in and calls[-1][3][1] is t_in
    apply_calibration_chain(vis, {"G": g_in, "T": t_in}, calibration_context="TG", inverse=True)
    assert calls[-1][1] == "TG" and calls[-1][4] is True      # a dict: context order
    apply_calibration_chain(vis, {"G": g_in, "T": t_in}, calibration_context="GT")
    assert calls[-1][1] == "GT"
    apply_calibration_chain(vis, t_in)
    assert calls[-1][1] == "T"
    controls = create_calibration_controls()
    controls["G"]["first_selfcal"] = 2
    apply_calibration_chain(vis, [g_in, t_in], calibration_context="TG", controls=controls,
                            iteration=1)
    assert calls[-1][1] == "T"
    n = len(calls)
    assert apply_calibration_chain(vis, [g_in, t_in], calibration_context="B") is vis
    controls["T"]["first_selfcal"] = 2
    apply_calibration_chain(vis, [g_in, t_in], calibration_context="TG", controls=controls,
                            iteration=1)
    assert len(calls) == n


def test_apply_calibration_chain_refuses_other_types(calls, caplog):
    g = golden("chain_apply_list.npz")
    vis, _ = cc.observation(g)
    with caplog.at_level(logging.WARNING, logger="func-python-logger"):
        assert apply_calibration_chain(vis, "T") is vis
    assert "Invalid GainTable format supplied. Visibility not updated." in caplog.text
    assert not calls


def test_qa_built_only_when_logged(calls, caplog, monkeypatch):
    g, vis, model, context, controls, iteration = _case("T_p1")
    made = []
    real = dm._GTAcc.qa_gain_table
    monkeypatch.setattr(dm._GTAcc, "qa_gain_table",
                        lambda self, context=None: made.append(context) or real(self, context))
    with caplog.at_level(logging.WARNING, logger="func-python-logger"):
        calibrate_chain(vis, model, calibration_context="T", controls=controls)
        solve_calibrate_chain(vis, model, calibration_context="T", controls=controls)
    assert not made
    with caplog.at_level(logging.DEBUG, logger="func-python-logger"):
        calibrate_chain(vis, model, calibration_context="T", controls=controls, iteration=2)
    assert made == ["Jones matrix T, iteration 2"]
    with caplog.at_level(logging.INFO, logger="func-python-logger"):
        solve_calibrate_chain(vis, model, calibration_context="T", controls=controls)
    assert len(made) == 2 and made[1].startswith("Model is non-zero: solving for Jones matrix T")
    assert "qa_gain_table" in caplog.text


# ---- gain-table operations ----------------------------------------------------
def _ops_table(gain, weight, time, nrec):
    return dm.GainTable.constructor(gain.copy(), time, np.full(len(time), 10.0), weight.copy(),
                                    np.zeros((len(time), gain.shape[2], nrec, nrec)),
                                    np.linspace(1e8, 1.1e8, gain.shape[2]),
                                    dm.PolarisationFrame("stokesI" if nrec == 1 else "linear"))


@pytest.mark.parametrize("nrec", [1, 2])
def test_multiply_gaintables_matches_reference(nrec):
    g = golden("gaintable_ops.npz")
    a = _ops_table(g[f"mul{nrec}_a_gain"], g[f"mul{nrec}_a_weight"], g["mul_time"], nrec)
    b = _ops_table(g[f"mul{nrec}_b_gain"], g[f"mul{nrec}_b_weight"], g["mul_time_b"], nrec)
    out = multiply_gaintables(a, b)
    assert out is a
    np.testing.assert_allclose(out["gain"].data, g[f"mul{nrec}_gain"], rtol=1e-14)
    np.testing.assert_allclose(out["weight"].data, g[f"mul{nrec}_weight"], rtol=1e-14)
    np.testing.assert_array_equal(b["gain"].data, g[f"mul{nrec}_b_gain"])
    if nrec == 2:   # the reference's product is gt^T dgt per matrix, not gt dgt
        want = np.swapaxes(g["mul2_a_gain"], -1, -2) @ g["mul2_b_gain"]
        np.testing.assert_allclose(out["gain"].data, want, rtol=1e-13)
        assert not np.allclose(out["gain"].data, g["mul2_a_gain"] @ g["mul2_b_gain"])


def test_multiply_gaintables_errors():
    g = golden("gaintable_ops.npz")
    a = _ops_table(g["mul1_a_gain"], g["mul1_a_weight"], g["mul_time"], 1)
    late = _ops_table(g["mul1_b_gain"], g["mul1_b_weight"], g["mul_time"] + 0.01, 1)
    with pytest.raises(ValueError, match=str(g["mul_error_time"])):
        multiply_gaintables(a, late)
    assert multiply_gaintables(a, late, time_tolerance=0.1) is a
    two = _ops_table(g["mul2_b_gain"], g["mul2_b_weight"], g["mul_time"], 2)
    with pytest.raises(ValueError, match=str(g["mul_error_structure"])):
        multiply_gaintables(a, two)
    ones = np.ones((3, 5, 3, 3, 3))
    three = _ops_table(ones.astype(complex), ones, g["mul_time"], 3)
    with pytest.raises(ValueError, match="illegal structures"):
        multiply_gaintables(three, three)


def test_concatenate_gaintables_round_trip():
    g = golden("gaintable_ops.npz")
    full = _ops_table(g["mul2_a_gain"], g["mul2_a_weight"], g["mul_time"], 2)
    full["residual"].data = np.random.default_rng(0).uniform(size=full["residual"].data.shape)
    full.attrs["jones_type"] = "B"

    def part(ts, fs):
        return dm.GainTable.constructor(
            full["gain"].data[ts, :, fs], full["time"].data[ts], full["interval"].data[ts],
            full["weight"].data[ts, :, fs], full["residual"].data[ts, fs],
            full["frequency"].data[fs], full.attrs["receptor_frame"], jones_type="B")

    for dim, parts in (("time", [part(slice(0, 1), slice(None)), part(slice(1, 3), slice(None))]),
                       ("frequency", [part(slice(None), slice(0, 2)),
                                      part(slice(None), slice(2, 3))])):
        out = concatenate_gaintables(parts, dim=dim)
        for k in cc.TABLE_VARS:
            np.testing.assert_array_equal(out[k].data, full[k].data, err_msg=f"{dim} {k}")
        assert out.attrs["jones_type"] == "B"
        assert out.attrs["receptor_frame"] == full.attrs["receptor_frame"]
    assert concatenate_gaintables([full])["gain"].data.shape == full["gain"].data.shape
    with pytest.raises(ValueError, match="GainTable list is empty"):
        concatenate_gaintables([])
    with pytest.raises(ValueError):
        concatenate_gaintables([full, full], dim="antenna")


def test_apply_jones_matches_reference():
    g = golden("gaintable_ops.npz")
    ej, cfs, small = g["jones_ej"], g["jones_cfs"], g["jones_small"]
    np.testing.assert_allclose(apply_jones(ej, cfs), g["jones_forward"], rtol=1e-14)
    np.testing.assert_allclose(apply_jones(ej, cfs, inverse=True), g["jones_inverse"], rtol=1e-14)
    below = apply_jones(small, cfs, inverse=True)
    np.testing.assert_array_equal(below, g["jones_below"])
    assert below.shape == cfs.shape and np.all(below == 0)
    np.testing.assert_allclose(apply_jones(small, cfs, inverse=True, min_det=1e-12),
                               g["jones_below_min_det"], rtol=1e-14)


def test_qa_gain_table_on_a_known_table():
    gain = np.zeros((2, 3, 1, 1, 1), complex)
    gain[0, :, 0, 0, 0] = [1.0, 2.0j, -3.0]
    gain[1, :, 0, 0, 0] = [4.0, 5.0, 100.0]
    weight = np.ones(gain.shape)
    weight[1, 2] = 0.0                      # the 100 does not count
    residual = np.array([0.25, 0.5]).reshape(2, 1, 1, 1)
    gt = dm.GainTable.constructor(gain, [0.0, 1.0], [1.0, 1.0], weight, residual, [1e8],
                                  dm.PolarisationFrame("stokesI"))
    qa = gt.gaintable_acc.qa_gain_table(context="known")
    assert qa.origin == "qa_gain_table" and qa.context == "known"
    amp = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    phase = np.array([0.0, np.pi / 2, np.pi, 0.0, 0.0])
    want = {"shape": (2, 3, 1, 1, 1), "maxabs-amp": 5.0, "minabs-amp": 1.0, "rms-amp": np.std(amp),
            "medianabs-amp": 3.0, "maxabs-phase": np.pi, "minabs-phase": 0.0,
            "rms-phase": np.std(phase), "medianabs-phase": 0.0, "residual": 0.5}
    assert set(qa.data) == set(want)
    for k, v in want.items():
        assert qa.data[k] == pytest.approx(v, rel=1e-15), k
    assert "qa_gain_table" in str(qa) and "known" in str(qa)


def test_timeslice_zero_none_auto_give_the_same_table():
    g = golden("chain_TG_p1.npz")
    vis, _ = cc.observation(g)
    tables = [dm.create_gaintable_from_visibility(vis, timeslice=ts, jones_type="T")
              for ts in (0.0, None, "auto", -1.0)]
    for t in tables[1:]:
        for k in cc.TABLE_VARS:
            np.testing.assert_array_equal(t[k].data, tables[0][k].data, err_msg=k)
    assert len(tables[0]["time"].data) == len(g["time"])
