"""GPU tests of the calibration chain: the one-pass gain-chain kernel
(sdp_hip_apply_gain_chain) against consecutive sdp_hip_apply_gains calls, bit
for bit, and calibrate_chain / solve_calibrate_chain / apply_calibration_chain
against the reference's own functions run on the same inputs
(tests/golden/chain_*.npz, written by tests/golden/make_golden_chain.py).

Bounds of the reference comparison.  A single solve_gaintable is pinned in
tests/test_gpu_solvers.py at TOL_G (gains, 1e-6 absolute = the solver's
stopping tolerance), TOL_W (gain weights) and TOL_R (residuals).  In
calibrate_chain the k-th solved letter is solved on visibilities that the k - 1
earlier solutions were taken off, so it absorbs their differences: k times
those bounds.  Every corrected visibility is divided by two gains per solved
letter, each within 1e-6: 2 k 1e-6 max|vis| after k letters.  The weights are
untouched by a non-singular gain: equal.  solve_calibrate_chain solves every
letter on the uncorrected visibilities: k = 1.  The forward
apply_calibration_chain fixtures hold two apply_gaintable calls, each pinned at
rtol 1e-12 in tests/test_gpu_calops.py: 2e-12.

Largest deviations measured on an MI355X (every test prints its own as
"DEV ..."; |dgain|, relative dweight, |dresidual|, and |dvis| / max|vis| of
the corrected visibilities):

                                   dgain    dweight  dresidual  dvis
  solve_calibrate_chain (k = 1)    6.0e-8   3.5e-8   1.4e-8     -
  calibrate_chain, 1st letter      3.7e-8   3.5e-8   8.2e-9     1.0e-8
  calibrate_chain, 2nd letter      3.8e-8   2.8e-8   4.1e-9     3.8e-8
  calibrate_chain, 3rd letter      4.1e-8   2.6e-8   5.9e-9     6.6e-9
  forward chain apply (relative)   -        -        -          1.8e-15

numpy and device-tensor inputs give the same figures.  The one-pass apply
equals the sequential calls bit for bit in every case (asserted).
"""

import numpy as np
import pytest
import torch

import chain_cases as cc
from conftest import golden
from test_gpu_solvers import TOL_G, TOL_R, TOL_W

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- the kernel contract: bit for bit the sequential calls ----------------------
def _tables(rng, nt, nants, nchan, npol, ntab, singular):
    """``ntab`` gain tables with their time-row maps.  Table 0: a row per
    time, one channel; table 1: a row per two times, nchan channels, time 1
    uncovered; table 2: one row, nchan channels; later ones: one row, one
    channel.  No table covers the last time.  ``singular``: table 1 (table 0
    of a single one) holds a gain without inverse; a scalar table 0 holds an
    exactly zero gain."""
    tables = []
    for k in range(ntab):
        nrow, nchan_g = [(nt, 1), ((nt + 1) // 2, nchan), (1, nchan)][k] if k < 3 else (1, 1)
        # npol 1 takes 2x2 tables too (the scalar Mueller sum runs over them)
        nrec = 2 if npol > 1 or k == 1 else 1
        shape = (nrow, nants, nchan_g, nrec, nrec)
        gain = rng.normal(1.0, 0.3, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))
        if npol == 2:
            gain[..., 0, 1] = gain[..., 1, 0] = 0.0
        tr = (np.arange(nt) * nrow // nt).astype(np.int32)
        if k == 1:
            tr[1] = -1
        tr[-1] = -1
        if singular and k == min(1, ntab - 1):
            if nrec == 2:
                gain[0, 1, 0] = np.array([[1.0, 2.0], [2.0, 4.0]])   # u22 = 4 - 2 * 2 = 0 exactly
            else:
                gain[0, 1, 0] = 0.0
        if nrec == 1 and k == 0:
            gain[0, 2, 0] = 0.0
        tables.append((torch.as_tensor(gain, device=DEV), torch.as_tensor(tr, device=DEV)))
    return tables


def _problem(nt, nbl, nchan, npol, dtype, seed):
    rng = np.random.default_rng(seed)
    nants = 2
    while nants * (nants - 1) // 2 < nbl:
        nants += 1
    a1, a2 = (x[:nbl].astype(np.int32) for x in np.triu_indices(nants, 1))
    shape = (nt, nbl, nchan, npol)
    vis = torch.as_tensor(rng.normal(size=shape) + 1j * rng.normal(size=shape), device=DEV)
    vis = vis.to(dtype)
    weight = torch.as_tensor(rng.uniform(0.5, 2.0, shape), device=DEV)
    return rng, nants, vis, weight, torch.as_tensor(a1, device=DEV), torch.as_tensor(a2, device=DEV)


def _sequential(vis, weight, a1, a2, tables, inverse):
    from ska_sdp_func_python_amd import kernels
    v, w = vis.clone(), weight.clone()
    for gain, tr in tables:
        kernels.apply_gains(v, w, None, False, a1, a2, tr, gain, inverse)
    return v, w


def _chain(vis, weight, a1, a2, tables, inverse):
    from ska_sdp_func_python_amd import kernels
    v, w = vis.clone(), weight.clone()
    kernels.apply_gain_chain(v, w, a1, a2, [t[1] for t in tables], [t[0] for t in tables], inverse)
    return v, w


# element counts (time x baseline x channel): below one workgroup of 256, an
# exact multiple, a multiple plus a tail
SHAPES = [(5, 10, 3), (8, 16, 4), (7, 21, 5)]


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("npol", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_chain_kernel_is_the_sequential_calls(shape, npol, dtype):
    nt, nbl, nchan = shape
    rng, nants, vis, weight, a1, a2 = _problem(nt, nbl, nchan, npol, dtype, seed=nt + npol)
    for ntab in (1, 2, 3):
        for inverse in (False, True):
            tables = _tables(rng, nt, nants, nchan, npol, ntab, singular=True)
            want_v, want_w = _sequential(vis, weight, a1, a2, tables, inverse)
            got_v, got_w = _chain(vis, weight, a1, a2, tables, inverse)
            tag = f"ntab {ntab} inverse {inverse}"
            assert torch.equal(got_v, want_v), tag
            assert torch.equal(got_w, want_w), tag
            # the time that no table covers is left as it was
            assert torch.equal(got_v[-1], vis[-1]) and torch.equal(got_w[-1], weight[-1])
            assert not torch.equal(got_v[0], vis[0])
            if inverse and npol == 4 and ntab >= 2:
                # the singular gain of antenna 1 (table 1, row 0, channel 0)
                # zeroes its baselines; the later table sees zeros
                hit = (a1 == 1) | (a2 == 1)
                assert torch.all(got_v[0, hit, 0] == 0) and torch.all(got_w[0, hit, 0] == 0)
                assert torch.all(got_w[0, ~hit, 0] != 0)
            if npol == 1 and ntab == 1:
                hit = (a1 == 2) | (a2 == 2)       # the exactly zero scalar gain
                assert torch.all(got_v[0, hit, 0] == 0) and torch.all(got_w[0, hit, 0] == 0)


@pytest.mark.parametrize("npol", [1, 2, 4])
def test_chain_kernel_unaligned_arrays(npol):
    """vis and weight 8 bytes off a 16-byte boundary: the element-wise path."""
    nt, nbl, nchan = 7, 21, 5
    rng, nants, vis, weight, a1, a2 = _problem(nt, nbl, nchan, npol, torch.complex64, seed=3)
    tables = _tables(rng, nt, nants, nchan, npol, 3, singular=False)
    want_v, want_w = _sequential(vis, weight, a1, a2, tables, True)
    from ska_sdp_func_python_amd import kernels
    vbuf = torch.empty(vis.numel() + 1, dtype=vis.dtype, device=DEV)
    wbuf = torch.empty(weight.numel() + 1, dtype=weight.dtype, device=DEV)
    v, w = vbuf[1:].view(vis.shape), wbuf[1:].view(weight.shape)
    assert v.data_ptr() % 16 == 8 and w.data_ptr() % 16 == 8
    v.copy_(vis)
    w.copy_(weight)
    kernels.apply_gain_chain(v, w, a1, a2, [t[1] for t in tables], [t[0] for t in tables], True)
    assert torch.equal(v, want_v) and torch.equal(w, want_w)


def test_chain_of_nine_tables_is_grouped():
    from ska_sdp_func_python_amd import kernels
    assert kernels.GAIN_CHAIN_MAX == 8
    nt, nbl, nchan = 5, 10, 3
    rng, nants, vis, weight, a1, a2 = _problem(nt, nbl, nchan, 4, torch.complex64, seed=9)
    tables = _tables(rng, nt, nants, nchan, 4, 9, singular=False)
    want_v, want_w = _sequential(vis, weight, a1, a2, tables, False)
    got_v, got_w = _chain(vis, weight, a1, a2, tables, False)
    assert torch.equal(got_v, want_v) and torch.equal(got_w, want_w)


def test_chain_kernel_refusals():
    from ska_sdp_func_python_amd import kernels
    rng, nants, vis, weight, a1, a2 = _problem(4, 6, 2, 4, torch.complex128, seed=1)
    with pytest.raises(ValueError, match="ntab"):
        kernels.apply_gain_chain(vis, weight, a1, a2, [], [], False)
    scalar = torch.ones((4, nants, 1, 1, 1), dtype=torch.complex128, device=DEV)
    tr = torch.arange(4, dtype=torch.int32, device=DEV)
    before = vis.clone()
    with pytest.raises(ValueError, match="2x2"):
        kernels.apply_gain_chain(vis, weight, a1, a2, [tr], [scalar], False)
    with pytest.raises(ValueError):
        kernels.apply_gain_chain(vis, weight, a1, a2, [tr[:3]], [scalar], False)
    assert torch.equal(vis, before)


# ---- the chain functions against the reference ------------------------------------
def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _check_table(tag, gt, g, prefix, k):
    got = [_host(gt[n].data) for n in ("gain", "weight", "residual")]
    want = [g[f"{prefix}_{n}"] for n in ("gain", "weight", "residual")]
    dw = np.max(np.abs(got[1] - want[1]) / np.maximum(np.abs(want[1]), 1e-300)
                * (np.abs(want[1]) > 0), initial=0.0)
    print(f"DEV {tag} k={k} dgain={np.max(np.abs(got[0] - want[0])):.3e} dweight_rel={dw:.3e} "
          f"dresidual={np.max(np.abs(got[2] - want[2])):.3e}")
    np.testing.assert_allclose(got[0], want[0], atol=k * TOL_G["atol"], rtol=0, err_msg=tag)
    np.testing.assert_allclose(got[1], want[1], rtol=k * TOL_W["rtol"], atol=k * TOL_W["atol"],
                               err_msg=tag)
    np.testing.assert_allclose(got[2], want[2], rtol=k * TOL_R["rtol"], atol=k * TOL_R["atol"],
                               err_msg=tag)


def _check_calibrated(tag, g, prefix, vis, model, context, controls, iteration, tables=None):
    """calibrate_chain against the fixture, and its corrected visibilities
    against apply_calibration_chain(inverse=True) of the returned tables."""
    from ska_sdp_func_python_amd.calibration import apply_calibration_chain, calibrate_chain
    original = vis.copy(deep=True)
    out, gt = calibrate_chain(vis, model, gaintables=tables, calibration_context=context,
                              controls=controls, iteration=iteration)
    assert out is vis
    assert sorted(gt) == sorted(str(g[f"{prefix}cal_letters"]))
    solved = [c for c in context if c in gt]
    for k, c in enumerate(solved, start=1):
        _check_table(f"{tag} calibrate {c}", gt[c], g, f"{prefix}cal_{c}", k)
    want = g[f"{prefix}cal_vis"]
    dv = np.max(np.abs(_host(out["vis"].data) - want)) / np.max(np.abs(want))
    print(f"DEV {tag} k={len(solved)} dvis_rel={dv:.3e}")
    assert dv <= 2 * len(solved) * 1e-6, tag
    np.testing.assert_array_equal(_host(out["weight"].data), g[f"{prefix}cal_weight"])
    again = apply_calibration_chain(original, gt, calibration_context=context, controls=controls,
                                    iteration=iteration, inverse=True)
    assert again is original
    np.testing.assert_array_equal(_host(again["vis"].data), _host(out["vis"].data))
    np.testing.assert_array_equal(_host(again["weight"].data), _host(out["weight"].data))
    return gt


def _check_solved(tag, g, prefix, vis, model, context, controls, iteration, tables=None):
    from ska_sdp_func_python_amd.calibration import solve_calibrate_chain
    before = _host(vis["vis"].data).copy()
    gt = solve_calibrate_chain(vis, model, gaintables=tables, calibration_context=context,
                               controls=controls, iteration=iteration)
    assert sorted(gt) == sorted(str(g[f"{prefix}sol_letters"]))
    for c in gt:
        _check_table(f"{tag} solve {c}", gt[c], g, f"{prefix}sol_{c}", 1)
    np.testing.assert_array_equal(_host(vis["vis"].data), before)   # nothing applied
    return gt


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("case", ["T_p1", "TG_p1", "TGB_p4", "GB_p2_gated"])
def test_chain_matches_reference(case, device):
    g = golden(f"chain_{case}.npz")
    context, controls, iteration = cc.settings(g)
    vis, model = cc.observation(g, device)
    _check_solved(f"{case}/{device}", g, "", vis, model, context, controls, iteration)
    gt = _check_calibrated(f"{case}/{device}", g, "", vis, model, context, controls, iteration)
    if case == "GB_p2_gated":
        assert list(gt) == ["G"]
    if case == "TGB_p4":
        assert gt["T"]["gain"].data.shape[2] == 1 and gt["B"]["gain"].data.shape[2] == 4


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("form", ["single", "list", "dict"])
def test_chain_existing_tables_match_reference(form, device):
    g = golden("chain_existing.npz")
    context, controls, iteration = cc.settings(g)

    def given(vis):
        t_in, g_in, b_in = (cc.table(g, f"in_{c}", c, vis) for c in "TGB")
        return {"single": t_in, "list": [g_in, t_in, b_in], "dict": {"T": t_in, "G": g_in}}[form]

    vis, model = cc.observation(g, device)
    _check_solved(f"existing {form}/{device}", g, f"{form}_", vis, model, context, controls,
                  iteration, given(vis))
    _check_calibrated(f"existing {form}/{device}", g, f"{form}_", vis, model, context, controls,
                      iteration, given(vis))


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_solve_calibrate_chain_without_weight_or_model(device):
    from ska_sdp_func_python_amd.calibration import solve_calibrate_chain
    g = golden("chain_solve_nomodel.npz")
    context, controls, iteration = cc.settings(g)
    vis, model = cc.observation(g, device)
    zero = vis.copy(deep=True)
    zero["weight"].data[...] = 0.0
    gt = solve_calibrate_chain(zero, model, calibration_context=context, controls=controls)
    for c in context:
        for n in ("gain", "weight", "residual"):
            np.testing.assert_array_equal(gt[c][n].data, g[f"zerowt_{c}_{n}"])
    gt = solve_calibrate_chain(vis, None, calibration_context=context, controls=controls)
    for c in context:
        _check_table(f"nomodel/{device} solve {c}", gt[c], g, f"nomodel_{c}", 1)


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("case", ["list", "gated", "nomatch"])
def test_apply_calibration_chain_matches_reference(case, device):
    from ska_sdp_func_python_amd.calibration import apply_calibration_chain
    g = golden(f"chain_apply_{case}.npz")
    context, controls, iteration = cc.settings(g)
    vis, _ = cc.observation(g, device)
    tables = [cc.table(g, f"in_{c}", c, vis) for c in str(g["list_order"])]
    out = apply_calibration_chain(vis, tables, calibration_context=context, controls=controls,
                                  iteration=iteration)
    assert out is vis
    got = _host(out["vis"].data)
    print(f"DEV apply {case}/{device} dvis_rel="
          f"{np.max(np.abs(got - g['out_vis']) / np.maximum(np.abs(g['out_vis']), 1e-300)):.3e}")
    np.testing.assert_allclose(got, g["out_vis"], rtol=2e-12, atol=2e-14)
    np.testing.assert_array_equal(_host(out["weight"].data), g["out_weight"])
    if case == "nomatch":
        np.testing.assert_array_equal(got, g["vis"])


def test_overlapping_windows_take_the_sequential_calls():
    """A table whose row windows overlap: apply_calibration_chain gives what
    consecutive apply_gaintable calls give (one launch per row there)."""
    from ska_sdp_func_python_amd.calibration import apply_calibration_chain, apply_gaintable
    g = golden("chain_apply_list.npz")
    vis, _ = cc.observation(g, True)
    want = vis.copy(deep=True)
    t_in, g_in = cc.table(g, "in_T", "T", vis), cc.table(g, "in_G", "G", vis)
    t_in["interval"].data = 3.0 * t_in["interval"].data
    for t in (g_in, t_in):
        apply_gaintable(want, t, inverse=True)
    out = apply_calibration_chain(vis, [g_in, t_in], calibration_context="TG", inverse=True)
    assert torch.equal(out["vis"].data, want["vis"].data)
    assert torch.equal(out["weight"].data, want["weight"].data)
    assert not torch.equal(out["vis"].data, torch.as_tensor(g["vis"], device=DEV))


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_device_visibilities_stay_where_they_are(dtype):
    from ska_sdp_func_python_amd.calibration import apply_calibration_chain, calibrate_chain
    g = golden("chain_TGB_p4.npz")
    context, controls, iteration = cc.settings(g)
    vis, model = cc.observation(g, True, dtype=dtype)
    ptrs = (vis["vis"].data.data_ptr(), vis["weight"].data.data_ptr())
    original = vis.copy(deep=True)
    out, gt = calibrate_chain(vis, model, calibration_context=context, controls=controls)
    assert out is vis and vis["vis"].data.is_cuda
    assert (vis["vis"].data.data_ptr(), vis["weight"].data.data_ptr()) == ptrs
    assert vis["vis"].data.dtype == original["vis"].data.dtype
    optrs = (original["vis"].data.data_ptr(), original["weight"].data.data_ptr())
    again = apply_calibration_chain(original, gt, calibration_context=context, inverse=True)
    assert again is original
    assert (original["vis"].data.data_ptr(), original["weight"].data.data_ptr()) == optrs
    # complex64 too: the one pass rounds between tables as the three calls did
    assert torch.equal(again["vis"].data, out["vis"].data)
    assert torch.equal(again["weight"].data, out["weight"].data)
