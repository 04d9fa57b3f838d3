"""CBF beamformer utilities on the host (calibration/beamformer_utils.py):
the host tables of the resamplers, applied by the numpy restatement of the two
kernels (tests/bandpass_restatement.py), and the public functions with the
kernel wrappers replaced by that restatement, against the reference's own
results (tests/golden/beamformer_*.npz).  The bounds are those of
tests/beamformer_cases.py.  Nothing here needs a GPU; the module does not
exist without the feature, so every test fails without it.
"""

import logging

import numpy as np
import pytest
import torch

import bandpass_restatement as br
import beamformer_cases as bc
from ska_sdp_func_python_amd.calibration import beamformer_utils as bu


def _fake_polyfit(gain, q, e, seg, edges):
    assert gain.is_contiguous() and gain.dtype == torch.complex128
    return torch.as_tensor(br.polyfit_apply(gain.numpy(), q, e, seg, edges))


def _fake_interp(gain, x_in, x_out, interval):
    assert gain.is_contiguous() and gain.dtype == torch.complex128
    return torch.as_tensor(br.interp_apply(gain.numpy(), x_in, x_out, interval))


@pytest.fixture
def host_layer(monkeypatch):
    from ska_sdp_func_python_amd import _device, kernels
    monkeypatch.setattr(_device, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(kernels, "resample_polyfit", _fake_polyfit)
    monkeypatch.setattr(kernels, "resample_interp", _fake_interp)


# ---- host tables, applied by the restatement ---------------------------------
@pytest.mark.parametrize("case", bc.RESAMPLE)
def test_polyfit_tables_reproduce_the_fixture(case):
    g = bc.load(f"resample_{case}")
    edges, deg = bc.resample_args(g)
    q, e, seg, ed = bu.polyfit_tables(g["frequency_out"], g["frequency"], edges,
                                      3 if deg is None else deg)
    assert q.dtype == e.dtype == np.float64 and seg.dtype == ed.dtype == np.int32
    assert np.array_equal(seg < 0, g["outside"])
    for k in range(len(ed) - 1):        # orthonormal on each segment's channels
        gram = q[:, ed[k]:ed[k + 1]] @ q[:, ed[k]:ed[k + 1]].T
        assert np.max(np.abs(gram - np.eye(len(q)))) < 64 * bc.EPS
    bc.check_polyfit(case, br.polyfit_apply(g["gain"], q, e, seg, ed), "tables")


@pytest.mark.parametrize("case", ["wide", "narrow", "mid", "lowband"])
def test_interp_and_spline_tables_reproduce_the_fixture(case):
    g = bc.load(f"resample_{case}")
    j = bu.interp_intervals(g["frequency_out"], g["frequency"])
    got = br.interp_apply(g["gain"], g["frequency"], g["frequency_out"], j)
    assert bc.same_bits(got, g["out_interp"])
    op = bu.spline_operator(g["frequency_out"], g["frequency"])
    bc.check_spline(case, br.spline_apply(op, g["gain"]), "tables")


def test_interp_intervals_follow_numpy_at_the_edges():
    x_in = np.array([1.0, 2.0, 4.0, 8.0])
    x_out = np.array([0.5, 1.0, 1.5, 2.0, 7.9, 8.0, 8.1, np.nan])
    assert list(bu.interp_intervals(x_out, x_in)) == [-1, 0, 0, 1, 2, 3, 3, -2]
    rng = np.random.default_rng(0)
    y = (rng.normal(size=(1, 1, 4, 1, 1)) + 1j * rng.normal(size=(1, 1, 4, 1, 1)))
    y[0, 0, 2, 0, 0] = np.nan + 1j * np.inf      # numpy's fallbacks
    got = br.interp_apply(y, x_in, x_out, bu.interp_intervals(x_out, x_in))[0, 0, :, 0, 0]
    assert bc.same_bits(got, np.interp(x_out, x_in, y[0, 0, :, 0, 0]))


# ---- the public functions over the restatement --------------------------------
@pytest.mark.parametrize("case", bc.RESAMPLE)
def test_resample_bandpass(case, host_layer, caplog):
    g = bc.load(f"resample_{case}")
    edges, deg = bc.resample_args(g)
    gt = bc.table(g["gain"], g["frequency"])
    with caplog.at_level(logging.WARNING, logger="func-python-logger"):
        got = bu.resample_bandpass(g["frequency_out"], gt, alg="polyfit", edges=edges, polydeg=deg)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex128
    assert got.shape == g["out_polyfit"].shape
    warned = [r for r in caplog.records if "no segment" in r.getMessage()]
    assert len(warned) == (1 if g["outside"].any() else 0)
    bc.check_polyfit(case, got, "host")
    if "interp" in str(g["algs"]):
        assert bc.same_bits(bu.resample_bandpass(g["frequency_out"], gt, alg="interp"),
                            g["out_interp"])
        bc.check_spline(case, bu.resample_bandpass(g["frequency_out"], gt, alg="cubicspl"), "host")


def test_resample_bandpass_takes_a_host_tensor_table(host_layer):
    g = bc.load("resample_narrow")
    gt = bc.table(g["gain"], g["frequency"], convert=torch.as_tensor)
    for alg in ("polyfit", "interp", "cubicspl"):
        got = bu.resample_bandpass(g["frequency_out"], gt, alg=alg)
        assert isinstance(got, np.ndarray)    # a host tensor is no device tensor
        assert got.shape == g[f"out_{alg}"].shape


def test_cubicspl_above_the_operator_limit_runs_scipy_on_the_host(host_layer, monkeypatch, caplog):
    g = bc.load("resample_narrow")
    monkeypatch.setattr(bu, "SPLINE_OPERATOR_MAX", 16)
    with caplog.at_level(logging.INFO, logger="func-python-logger"):
        got = bu.resample_bandpass(g["frequency_out"], bc.table(g["gain"], g["frequency"]),
                                   alg="cubicspl")
    assert any("host copy" in r.getMessage() for r in caplog.records)
    bc.check_spline("narrow", got, "host scipy")


def test_resample_refusals(host_layer):
    g = bc.load("resample_narrow")
    gt = bc.table(g["gain"], g["frequency"])
    f_out = g["frequency_out"]
    with pytest.raises(ValueError, match="unknown resampler"):
        bu.resample_bandpass(f_out, gt, alg="nearest")
    with pytest.raises(ValueError, match="degrees 0 to 7"):
        bu.resample_bandpass(f_out, gt, polydeg=8)
    with pytest.raises(ValueError, match="degrees 0 to 7"):
        bu.resample_bandpass(f_out, gt, polydeg=-1)
    with pytest.raises(ValueError, match="no more channels than polydeg"):
        bu.resample_bandpass(f_out, gt, edges=[0, 3], polydeg=3)   # a segment of 3 channels
    with pytest.raises(ValueError, match="ascend"):
        bu.resample_bandpass(f_out, gt, edges=[0, 40, 20])
    with pytest.raises(ValueError, match="at most 64"):
        bu.polyfit_tables(np.arange(10.0), np.arange(130.0), list(range(0, 130, 2)), 0)
    one = bc.table(g["gain"][:, :, :1], g["frequency"][:1])
    with pytest.raises(ValueError, match="at least 2"):
        bu.resample_bandpass(f_out, one)
    # exactly polydeg + 1 channels in a segment is a fit (an interpolation)
    got = bu.resample_bandpass(g["frequency"][:4], gt, edges=[0, 4], polydeg=3)
    assert np.max(np.abs(got[:, :, :4] - g["gain"][:, :, :4])) < 1e-12


def test_set_edges_normalisation():
    p = bu.PolynomialInterpolator()
    assert p.edges is None and p.polydeg == 3
    for given, want in ((None, [0, 96]), ([], [0, 96]), ([0, 30, 61], [0, 30, 61, 96]),
                        ([30, 61], [0, 30, 61, 96]), ([0, 96], [0, 96]), ([30], [0, 30, 96]),
                        (np.array([30, 61]), [0, 30, 61, 96])):
        p.set_edges(given, 96)
        assert list(p.edges) == want
    p.set_polydeg(5)
    assert p.polydeg == 5


def test_interpolator_classes_keep_the_reference_interface():
    g = bc.load("resample_edges")
    edges, deg = bc.resample_args(g)
    spectrum = g["gain"][1, 2, :, 0, 1]
    p = bu.PolynomialInterpolator()
    p.set_edges(edges, len(spectrum))
    p.set_polydeg(deg)
    got = p.interp(g["frequency_out"], g["frequency"], spectrum)
    tight, rounding, ref_bound, outside = bc.polyfit_yardstick("edges")
    assert np.all(np.isnan(got[outside]))
    assert np.all(np.abs(got - g["out_polyfit"][1, 2, :, 0, 1])[~outside]
                  <= ref_bound[1, 2, :, 0, 1][~outside])
    w = bc.load("resample_wide")
    spectrum = w["gain"][0, 1, :, 1, 0]
    got = bu.PolynomialInterpolator().interp(w["frequency_out"], w["frequency"], spectrum)
    assert np.all(np.abs(got - w["out_polyfit"][0, 1, :, 1, 0])
                  <= bc.polyfit_yardstick("wide")[2][0, 1, :, 1, 0])
    got = bu.NumpyLinearInterpolator().interp(w["frequency_out"], w["frequency"], spectrum)
    assert bc.same_bits(got, w["out_interp"][0, 1, :, 1, 0])
    got = bu.ScipySplineInterpolator().interp(w["frequency_out"], w["frequency"], spectrum)
    assert bc.same_bits(got, w["out_cubicspl"][0, 1, :, 1, 0])


# ---- frequencies, delays, products --------------------------------------------
def test_set_beamformer_frequencies(caplog):
    g = bc.load("frequencies")
    for k in ("low", "mid", "one", "unknown", "forced"):
        f_in = g[f"{k}_in"]
        gt = bc.table(np.ones((2, 3, len(f_in), 2, 2), complex), f_in, name=str(g[f"{k}_name"]))
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="func-python-logger"):
            got = bu.set_beamformer_frequencies(gt, array=str(g[f"{k}_array"]) or None)
        assert bc.same_bits(np.asarray(got), g[f"{k}_out"])
        assert len(caplog.records) == (1 if k in ("one", "unknown") else 0)
    assert np.all(g["low_out"] % 781.25e3 == 0)


def test_expand_delay_phase():
    g = bc.load("expand")
    gt = bc.table(g["gain"], g["frequency0"], "K")
    for tag, centre in (("centre", True), ("raw", False)):
        for frequency in (g["frequency"].copy(), list(g["frequency"])):
            keep = np.array(frequency)
            got = bu.expand_delay_phase(gt, frequency, reference_to_centre=centre)
            assert np.array_equal(np.array(frequency), keep)     # the caller's is only read
            assert got.jones_type == "B"
            assert bc.same_bits(got.gain.data, g[f"out_{tag}"])
            assert np.all(got.weight.data == 1) and got.weight.data.shape == got.gain.data.shape
            assert np.all(got.residual.data == 0) and got.residual.data.shape == (3, 5, 2, 2)
            assert np.array_equal(got.frequency.data, g["frequency"])
    with pytest.raises(ValueError, match=str(g["error_type"])):
        bu.expand_delay_phase(bc.table(g["gain"], g["frequency0"], "B"), g["frequency"])
    with pytest.raises(ValueError, match=str(g["error_frequency"])):
        bu.expand_delay_phase(bc.table(np.repeat(g["gain"], 2, 2), [1.5e8, 1.6e8], "K"),
                              g["frequency"])


@pytest.mark.parametrize("run", bc.MULTIPLY)
def test_multiply_gaintable_jones(run):
    g = bc.load("multiply")
    a, b, elem = (str(v) for v in g[f"run_{run}"])
    t1, t2 = bc.multiply_table(g, a), bc.multiply_table(g, b)
    keep = t1.gain.data.copy()
    got = bu.multiply_gaintable_jones(t1, t2, elementwise=elem == "1")
    assert np.array_equal(t1.gain.data, keep)
    want = g[f"{run}_out_gain"]
    if elem == "1":
        assert bc.same_bits(got.gain.data, want)
    else:
        assert got.gain.data.shape == want.shape
        assert np.all(np.abs(got.gain.data - want) <= bc.product_bound(t1.gain.data, t2.gain.data))
    assert got.jones_type == str(g[f"{run}_out_jones"])
    for v in ("weight", "residual", "frequency"):
        assert bc.same_bits(np.asarray(got[v].data), g[f"{run}_out_{v}"])


def test_multiply_refusals():
    g = bc.load("multiply")
    b5, bs5, g1 = (bc.multiply_table(g, k) for k in ("B5", "Bs5", "G1"))
    cut = lambda t, s: bc.table(t.gain.data[s], t.frequency.data[:t.gain.data[s].shape[2]])  # noqa
    cases = {
        "K": (bc.table(g1.gain.data, g1.frequency.data, "K"), b5, False),
        "time": (cut(b5, np.s_[:2]), b5, False),
        "antenna": (cut(b5, np.s_[:, :3]), b5, False),
        "frequency": (cut(b5, np.s_[:, :, :3]), b5, False),
        "pol": (bs5, b5, True),
        "matrix": (b5, bs5, False),
    }
    for k, (t1, t2, elem) in cases.items():
        with pytest.raises(ValueError, match=str(g[f"error_{k}"])):
            bu.multiply_gaintable_jones(t1, t2, elementwise=elem)


def test_exports():
    from ska_sdp_func_python_amd import calibration
    for name in ("set_beamformer_frequencies", "expand_delay_phase", "multiply_gaintable_jones",
                 "resample_bandpass"):
        assert getattr(calibration, name) is getattr(bu, name)
