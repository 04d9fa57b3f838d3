"""GPU parity of solve_gaintable (batched StefCal, sdp_hip_solve_gains)
against the reference's own solve_gaintable run on the same inputs
(tests/golden/solve_*.npz), and of kernels.solve_gains against the restated
reference solver (oracle/ref_oracle.stefcal_row).

The kernel stores the normalised point-source vis / weights in fp32 and
iterates in fp64.  A relative perturbation of 6e-8 in x moves the fixed point
of the substitution g_j = sum_i g_i x_ij w_ij / sum_i |g_i|^2 w_ij by the same
relative order, far below the reference's stopping tolerance tol = 1e-6, so
the stopping iteration and the gains agree: measured max |dgain| 4.5e-8 over
the seven fixtures, 6e-9 on 512-station C5 rows with equal iteration counts
(scripts/gpu_stefcal_parity.py, tests/test_gpu_fullsize.py).  Asserted:
gains to 1e-6 absolute (= tol), weights to 1e-6 relative, residuals to 1e-7.

What is pinned beyond the seven tidy fixtures (all at those tolerances):

* solve_gaintable on ragged tables (solve_ragged_*.npz: autocorrelations,
  one of them with the row's largest weight; shuffled baselines, half given
  as (a2, a1); weights, flags, a wholly flagged time, a gain row outside
  every time, a starting table that is not all ones; 65-67 antennas), with
  numpy and device-tensor inputs and with complex64 vis / model;
* the column blocks of k_iter at every edge (2 ... 1024 antennas, scalar) and
  in the 2x2 modes across 2, 3 and 5 blocks, the row maximum in a cross hand;
* rows of one batch that stop at their own iteration, niter = 0;
* refant, damping; both k_fill tiles at the switch; scratch reuse; refusals.

Largest deviations measured on an MI355X per group (|dgain|, relative
dweight, |dresidual|; every test prints its own as "DEV ..."):

  ragged fixtures                  9.7e-9   1.1e-8   7.5e-10
  ... device-tensor inputs         5.4e-9   9.7e-9   7.5e-10
  ... complex64, vs oracle on the
      rounded inputs (asserted)    1.3e-8   8.0e-9   4.7e-10
  ... complex64, vs fp64 fixture   2.4e-8   6.4e-8   2.5e-10
  block edges, scalar              6.7e-8   7.3e-8   7.8e-10
  2x2 modes across blocks          1.6e-8   1.8e-8   1.7e-9
  stopping batches                 1.8e-8   1.5e-8   2.1e-9
  niter = 0                        3.4e-16  0        1.6e-9
  refant / damping                 1.2e-8   9.4e-9   8.0e-10
  fill tiles                       3.5e-8   3.5e-8   4.8e-9
  scratch reuse                    2.4e-8   1.4e-8   9.7e-10
"""

import numpy as np
import pytest

from conftest import golden
from gpu_helpers import vis_from_arrays

pytestmark = pytest.mark.gpu

RAGGED = ["ragged_scalar_T_median", "ragged_matrix_B", "ragged_nocross_T"]
CASES = ["scalar_T_phase", "scalar_B_amp_mean", "scalar_T_amp_median", "matrix_crosspol_B",
         "nocross_linear_T", "nocross_linearnp_B", "nocross_circular_T"] + RAGGED

TOL_G = dict(atol=1e-6)
TOL_W = dict(rtol=1e-6, atol=1e-12)
TOL_R = dict(rtol=1e-5, atol=1e-7)


def _devs(group, got, want):
    """Print the largest |dgain|, relative dweight and dresidual of a case
    (DESIGN.md section 5 records them) before the caller asserts."""
    (gg, gw, gr), (eg, ew, er) = got, want
    dw = np.max(np.abs(gw - ew) / np.maximum(np.abs(ew), 1e-300) * (np.abs(ew) > 0), initial=0.0)
    print(f"DEV {group} dgain={np.max(np.abs(gg - eg)):.3e} dweight_rel={dw:.3e} "
          f"dresidual={np.max(np.abs(gr - er)):.3e}")


def _check(group, got, want):
    _devs(group, got, want)
    np.testing.assert_allclose(got[0], want[0], **TOL_G)
    np.testing.assert_allclose(got[1], want[1], **TOL_W)
    np.testing.assert_allclose(got[2], want[2], **TOL_R)


def _tables(g):
    from ska_sdp_func_python_amd import datamodels as dm
    pf = str(g["pol_frame"])
    ragged = "vis_weight" in g
    vis = vis_from_arrays(g["uvw"], g["frequency"], g["vis"], baselines=g["baselines"], pf=pf,
                          times=g["time"], integration_time=g["integration_time"],
                          weight=g["vis_weight"].copy() if ragged else None,
                          flags=g["vis_flags"].astype(np.int64) if ragged else None)
    model = vis.copy(deep=True)
    model["vis"].data = g["model"].copy()
    if ragged:  # the table has a row beyond the visibility's times
        nrec = g["gain_in"].shape[-1]
        gt = dm.GainTable.constructor(
            g["gain_in"].copy(), g["gt_time"], g["gt_interval"], g["weight_in"].copy(),
            g["residual_in"].copy(), g["gt_frequency"],
            dm.PolarisationFrame("stokesI" if nrec == 1 else "linear"), jones_type=str(g["jones"]))
        return vis, model, gt
    gt = dm.create_gaintable_from_visibility(vis, jones_type=str(g["jones"]))
    gt["gain"].data = g["gain_in"].copy()
    gt["weight"].data = g["weight_in"].copy()
    return vis, model, gt


def _solve_fixture(g, vis, model, gt):
    from ska_sdp_func_python_amd.calibration import solve_gaintable
    norm = str(g["normalise"])
    return solve_gaintable(vis, model, gain_table=gt, phase_only=bool(g["phase_only"]),
                           niter=int(g["niter"]), tol=float(g["tol"]), crosspol=bool(g["crosspol"]),
                           normalise_gains=None if norm == "None" else norm,
                           jones_type=str(g["jones"]))


@pytest.mark.parametrize("case", CASES)
def test_solve_gaintable_matches_reference(case):
    g = golden(f"solve_{case}.npz")
    vis, model, gt = _tables(g)
    out = _solve_fixture(g, vis, model, gt)
    for k in ("gain", "weight", "residual"):
        assert isinstance(out[k].data, np.ndarray)  # numpy in, numpy out
    _devs(f"2/{case}", [out[k].data for k in ("gain", "weight", "residual")],
          [g[k] for k in ("gain", "weight", "residual")])
    np.testing.assert_allclose(out["gain"].data, g["gain"], atol=1e-6)
    np.testing.assert_allclose(out["weight"].data, g["weight"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(out["residual"].data, g["residual"], rtol=1e-5, atol=1e-7)


def test_solve_gaintable_device_tensor_inputs():
    """vis, model, weight and flags handed over as device tensors (the gain
    table stays numpy): the same table as from numpy inputs, and the gain
    table's arrays come back as the kind they went in."""
    import torch
    g = golden("solve_ragged_matrix_B.npz")
    vis, model, gt = _tables(g)
    for k in ("vis", "weight", "flags"):
        vis[k].data = torch.as_tensor(vis[k].data, device="cuda")
    model["vis"].data = torch.as_tensor(model["vis"].data, device="cuda")
    model["flags"].data = vis["flags"].data
    out = _solve_fixture(g, vis, model, gt)
    for k in ("gain", "weight", "residual"):
        assert isinstance(out[k].data, np.ndarray)
    _check("2/ragged_matrix_B/device", [out[k].data for k in ("gain", "weight", "residual")],
           [g[k] for k in ("gain", "weight", "residual")])


def test_solve_gaintable_complex64_visibilities():
    """complex64 vis and model: the driver forms the point-source sums from
    them in fp64, so the table is that of the oracle run on the rounded
    values, to the float32 bound tests/test_gpu_calops.py asserts for
    complex64 inputs (1e-6).  Rounding the inputs itself moves the gains by
    the printed "vs fp64 fixture" figure."""
    import calops_oracle as co
    g = golden("solve_ragged_scalar_T_median.npz")
    vis, model, gt = _tables(g)
    vis["vis"].data = vis["vis"].data.astype(np.complex64)
    model["vis"].data = model["vis"].data.astype(np.complex64)
    want = co.solve_gaintable_fixture(g, vis=vis["vis"].data.astype(complex),
                                      model=model["vis"].data.astype(complex))
    out = _solve_fixture(g, vis, model, gt)
    got = [out[k].data for k in ("gain", "weight", "residual")]
    _devs("2/ragged_scalar_T_median/complex64 vs fp64 fixture", got,
          [g[k] for k in ("gain", "weight", "residual")])
    _devs("2/ragged_scalar_T_median/complex64", got, want)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got[1], want[1], **TOL_W)
    np.testing.assert_allclose(got[2], want[2], **TOL_R)


def test_zero_model_raises():
    from ska_sdp_func_python_amd.calibration import solve_gaintable
    g = golden("solve_scalar_T_phase.npz")
    vis, model, gt = _tables(g)
    model["vis"].data[...] = 0.0
    with pytest.raises(ValueError):
        solve_gaintable(vis, model)


def test_recovers_simulated_gains_large():
    """512 antennas, 4 channels jointly: the solved phases match the truth up
    to the refant rotation (residual bound, cf. reference
    tests/calibration/test_chain_calibration.py:126-127)."""
    import torch
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(1805550721)
    nants, nchan = 512, 4
    a1, a2 = np.triu_indices(nants, 1)
    g = np.exp(1j * rng.normal(0, 0.5, (nants, nchan)))
    xb = (g[a1] * np.conj(g[a2]))[None, :, :, None]
    wb = np.ones_like(xb.real)
    perm, conj, rs, ant2 = kernels.canonical_baselines(a1, a2, nants)
    dev = torch.device("cuda:0")
    gain = torch.ones((1, nants, nchan, 1, 1), dtype=torch.complex128, device=dev)
    gwt = torch.zeros((1, nants, nchan, 1, 1), dtype=torch.float64, device=dev)
    res, used = kernels.solve_gains(torch.as_tensor(xb[:, perm], device=dev),
                                    torch.as_tensor(wb[:, perm], device=dev), gain, gwt, rs, ant2,
                                    mode=0, niter=200, tol=1e-8, phase_only=True)
    sol = gain.cpu().numpy()[0, :, :, 0, 0]
    truth = g * np.exp(-1j * np.angle(g[0]))[None, :]
    assert np.max(np.abs(sol - truth)) < 1e-5
    assert float(res.max()) < 1.3e-6
    assert int(used[0]) <= 200


@pytest.mark.parametrize("nants", [37, 300])
def test_irregular_baselines_match_oracle(nants):
    """A sparse, ragged baseline set (60 % of the pairs, one antenna with no
    baselines at all, so CSR rows of every length and empty rows) with noisy
    data and random weights, two gain rows: the device solve against the
    restated reference solver (oracle/ref_oracle.stefcal_row) iteration for
    iteration (fixed niter, no early stop)."""
    import torch
    import ref_oracle as ro
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(nants)
    nchan = 3
    a1, a2 = np.triu_indices(nants, 1)
    keep = (rng.uniform(size=a1.size) < 0.6) & (a1 != 7) & (a2 != 7)
    a1, a2 = a1[keep], a2[keep]
    g = np.exp(1j * rng.normal(0, 0.5, (nants, nchan))) * rng.uniform(0.8, 1.2, (nants, nchan))
    nsolve = 2
    xb = np.stack([(g[a1] * np.conj(g[a2])) * (1 + 0.05 * s) for s in range(nsolve)])[..., None]
    xb = xb + 0.02 * (rng.normal(size=xb.shape) + 1j * rng.normal(size=xb.shape))
    wb = rng.uniform(0.5, 2.0, xb.shape)
    perm, conj, rs, ant2 = kernels.canonical_baselines(a1, a2, nants)
    assert not np.any(conj)
    dev = torch.device("cuda:0")
    gain = torch.ones((nsolve, nants, nchan, 1, 1), dtype=torch.complex128, device=dev)
    gwt = torch.zeros((nsolve, nants, nchan, 1, 1), dtype=torch.float64, device=dev)
    res, used = kernels.solve_gains(torch.as_tensor(xb[:, perm], device=dev),
                                    torch.as_tensor(wb[:, perm], device=dev), gain, gwt, rs, ant2,
                                    mode=0, niter=12, tol=0.0, phase_only=False)
    bl = list(zip(a1, a2))
    for s in range(nsolve):
        eg, ew, er, eu = ro.stefcal_row(xb[s], wb[s], bl, nants,
                                        np.ones((nants, nchan, 1, 1), complex),
                                        np.zeros((nants, nchan, 1, 1)), niter=12, tol=0.0,
                                        phase_only=False)
        assert int(used[s]) == eu
        np.testing.assert_allclose(gain[s].cpu().numpy(), eg, atol=1e-6)
        np.testing.assert_allclose(gwt[s].cpu().numpy(), ew, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(res[s].cpu().numpy(), er, rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------
# kernels.solve_gains against ref_oracle.stefcal_row on ragged baseline sets
# ---------------------------------------------------------------------------

def _ragged(nants, nchan, npol, nsolve, seed, cross_heavy=False):
    """60 % of the pairs, one antenna (7, or the last of 3) without any, true
    gains with noise 0.02, weights in [0.5, 2], 5 % of the kept baselines with
    weight 0 in one channel only.  x_b is the weighted sum the driver would
    hand over (x w).  ``cross_heavy`` puts each row's largest weight into a
    cross-hand pol (npol 4)."""
    rng = np.random.default_rng(seed)
    a1, a2 = np.triu_indices(nants, 1)
    lonely = 7 if nants > 8 else (2 if nants == 3 else -1)
    keep = (rng.uniform(size=a1.size) < 0.6) & (a1 != lonely) & (a2 != lonely)
    keep[0] = True  # (0, 1): never empty
    a1, a2 = a1[keep], a2[keep]
    g = np.exp(1j * rng.normal(0, 0.5, (nants, nchan, npol))) * rng.uniform(0.8, 1.2, (nants, nchan, npol))
    x = np.stack([(g[a1] * np.conj(g[a2])) * (1 + 0.05 * s) for s in range(nsolve)])
    if npol == 4:
        x[..., 1:3] *= 0.1
    x = x + 0.02 * (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape))
    wb = rng.uniform(0.5, 2.0, x.shape)
    dead = np.nonzero(rng.uniform(size=a1.size) < 0.05)[0]
    wb[:, dead, rng.integers(0, nchan, dead.size)] = 0.0
    if cross_heavy:
        for s in range(nsolve):
            wb[s, 3 + s, 0, 1 + (s & 1)] = 3.0
    return dict(a1=a1, a2=a2, xb=x * wb, wb=wb, nants=nants, nchan=nchan, npol=npol, nsolve=nsolve,
                lonely=lonely, nrec=1 if npol == 1 else 2)


def _start(c, gain0=None, gwt0=None):
    shape = (c["nsolve"], c["nants"], c["nchan"], c["nrec"], c["nrec"])
    gain0 = np.ones(shape, complex) if gain0 is None else gain0
    gwt0 = np.zeros(shape) if gwt0 is None else gwt0
    return gain0, gwt0


def _device_solve(c, mode, niter, tol=0.0, phase_only=False, gain0=None, gwt0=None, **kw):
    import torch
    from ska_sdp_func_python_amd import kernels
    perm, conj, rs, ant2 = kernels.canonical_baselines(c["a1"], c["a2"], c["nants"])
    assert not np.any(conj)
    gain0, gwt0 = _start(c, gain0, gwt0)
    gain = torch.as_tensor(gain0, device="cuda").clone()
    gwt = torch.as_tensor(gwt0, device="cuda").clone()
    res, used = kernels.solve_gains(torch.as_tensor(c["xb"][:, perm], device="cuda"),
                                    torch.as_tensor(c["wb"][:, perm], device="cuda"), gain, gwt,
                                    rs, ant2, mode=mode, niter=niter, tol=tol,
                                    phase_only=phase_only, **kw)
    return gain.cpu().numpy(), gwt.cpu().numpy(), res.cpu().numpy(), used.cpu().numpy()


def _oracle_solve(c, mode, niter, tol=0.0, phase_only=False, gain0=None, gwt0=None, changes=None,
                  **kw):
    import ref_oracle as ro
    gain0, gwt0 = _start(c, gain0, gwt0)
    bl = list(zip(c["a1"], c["a2"]))
    out = [ro.stefcal_row(c["xb"][s], c["wb"][s], bl, c["nants"], gain0[s], gwt0[s], niter=niter,
                          tol=tol, phase_only=phase_only, crosspol=mode == 1,
                          changes=None if changes is None else changes[s], **kw)
           for s in range(c["nsolve"])]
    return [np.array([o[k] for o in out]) for k in range(4)]


def _parity(group, c, mode, niter, **kw):
    got = _device_solve(c, mode, niter, **kw)
    want = _oracle_solve(c, mode, niter, **kw)
    np.testing.assert_array_equal(got[3], want[3])
    _check(group, got[:3], want[:3])
    return got, want


@pytest.mark.parametrize("nants", [2, 3, 63, 64, 65, 128, 129, 257, 513, 1024])
def test_block_edges_scalar(nants):
    """Column blocks of 64 antennas with rows(c) = min(64 c + 63, nants - 1):
    one block with 1, 2, 62 and 63 rows (2, 3, 63, 64 antennas), a second block
    of one antenna with 64 rows (65), two full blocks (128: 63 and 127 rows),
    a third of one antenna with 128 rows (129), 5 and 9 blocks (257, 513:
    snake rounds 1 and 2, a last block of one antenna with 256 / 512 rows)
    and the ABI's limit (1024: 16 blocks, snake rounds 0-3, 1023 rows).
    The row loop takes 16 rows per turn in two halves of 8 and prefetches up
    to 16 rows past the end, clamped and masked.  Its last turn differs by
    rows % 16: 1-8 runs the first half only (1, 2: these sizes), 9-15 both
    with the second partly masked (14: 62 rows; 15: 63, 127, ... 1023 rows,
    every full block), 0 both in full (64, 128, 256, 512 rows).  All three
    classes are in this list.  Complex gains, 6 iterations, no stop."""
    nchan, nsolve = (1, 1) if nants == 1024 else (2, 2)
    c = _ragged(nants, nchan, 1, nsolve, seed=1000 + nants)
    _parity(f"3a/{nants}", c, 0, 6)


@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("nants", [65, 130, 257])
@pytest.mark.parametrize("mode,npol", [(1, 4), (2, 2), (2, 4)])
def test_blocks_2x2_modes(mode, npol, nants, phase_only):
    """The element-wise 2x2 solvers across 2, 3 and 5 column blocks (a last
    block of 1, 2 and 1 antennas).  Mode 2 with 4 pols carries each row's
    largest weight in a cross hand: the reference normalises by the maximum
    over all pols before it drops the cross hands (solvers.py:167), which
    scales the returned gain weights.  The cross-hand gains come back 0; their
    residual is the weighted rms of x in mode 1 and 0 in mode 2, as the oracle
    has them."""
    c = _ragged(nants, 2, npol, 2, seed=2000 + 10 * nants + npol + mode,
                cross_heavy=(mode == 2 and npol == 4))
    if mode == 2 and npol == 4:
        for s in range(2):
            assert np.unravel_index(np.argmax(c["wb"][s]), c["wb"][s].shape)[-1] in (1, 2)
    got, want = _parity(f"3b/mode{mode}_npol{npol}_{nants}_po{int(phase_only)}", c, mode, 8,
                        phase_only=phase_only)
    assert np.all(got[0][..., 0, 1] == 0) and np.all(got[0][..., 1, 0] == 0)
    assert np.all(want[0][..., 0, 1] == 0) and np.all(want[0][..., 1, 0] == 0)
    if mode == 1:
        assert want[2][..., 0, 1].min() > 0.01  # rms of the cross-hand x
    else:
        assert np.all(got[2][..., 0, 1] == 0) and np.all(got[2][..., 1, 0] == 0)


STOP_TOL = 1e-4
STOP_NITER = 12
# relative distance of each row's starting gains from its own solution (None:
# all ones); chosen on the CPU so that the oracle's iteration counts meet
# _stop_batch's conditions in both phase_only settings
STOP_EPS = {0: (1e-5, 1.2e-3, 3e-3, None, 6e-3, 2.5e-2),
            1: (1e-5, 8e-4, 1.5e-3, None, 1.2e-2, 1.8e-2, 2.5e-2)}


def _stop_batch(mode, npol, phase_only):
    """65 antennas, one batch of rows that start at different distances from
    their solutions, tol 1e-4, 12 iterations (host polls after 4, 8 and 12).
    Returns the case, the starting gains, the oracle's answers; asserts from
    the oracle alone that the batch holds: a row done before the first poll,
    one done exactly at a poll, one between polls, one that runs out, a row
    going on for >= 4 iterations after another froze, and no change value
    within 5 % of tol (the device's fp32 x shifts change by ~1e-7, 0.1 % of
    tol, so the stopping iterations are the oracle's)."""
    eps = STOP_EPS[mode]
    c = _ragged(65, 2, npol, len(eps), seed=3000 + mode)
    rng = np.random.default_rng(77)
    sol = _oracle_solve(c, mode, 400, tol=1e-13, phase_only=phase_only)[0]
    pert = rng.normal(size=sol.shape) + 1j * rng.normal(size=sol.shape)
    gain0 = np.ones_like(sol)
    for s, e in enumerate(eps):
        if e is not None:
            gain0[s] = sol[s] * (1 + e * pert[s])
            # the antenna without baselines: its gain only halves per
            # iteration (damping), 14 of them from 1 down to tol
            gain0[s, c["lonely"]] = 0.0
    gwt0 = rng.uniform(0.5, 1.5, sol.shape)
    changes = [[] for _ in eps]
    want = _oracle_solve(c, mode, STOP_NITER, tol=STOP_TOL, phase_only=phase_only, gain0=gain0,
                         gwt0=gwt0, changes=changes)
    used = want[3]
    allch = np.concatenate([np.array(ch) for ch in changes])
    assert not np.any(np.abs(allch - STOP_TOL) < 0.05 * STOP_TOL), (used, sorted(allch))
    assert np.any(used <= 3), used
    assert np.any(np.isin(used, (4, 8, 12))), used
    assert np.any((used > 4) & (used % 4 != 0) & (used <= STOP_NITER)), used
    assert np.any(used == STOP_NITER + 1), used
    assert used.max() - used.min() >= 4
    return c, gain0, gwt0, want


@pytest.mark.parametrize("phase_only", [False, True])
@pytest.mark.parametrize("mode,npol", [(0, 1), (1, 4)])
def test_rows_stop_at_their_own_iteration(mode, npol, phase_only):
    """Rows of one batch freeze at the oracle's iteration each, whatever their
    neighbours do, and keep the gains, gain weights and residual of that
    iteration: done[] in k_iter / k_commit / k_mark_done, the poll every 4th
    iteration, the double-buffered change array, the phase-only normalisation
    on convergence and on running out (solvers.py:270-272, :280-282)."""
    c, gain0, gwt0, want = _stop_batch(mode, npol, phase_only)
    got = _device_solve(c, mode, STOP_NITER, tol=STOP_TOL, phase_only=phase_only, gain0=gain0,
                        gwt0=gwt0)
    print("used", got[3], want[3])
    np.testing.assert_array_equal(got[3], want[3])
    for s in range(c["nsolve"]):
        _check(f"3c/mode{mode}_po{int(phase_only)}/row{s}", [a[s] for a in got[:3]],
               [a[s] for a in want[:3]])


@pytest.mark.parametrize("phase_only", [False, True])
def test_niter_zero_returns_the_input(phase_only):
    """No iteration: the gains as given (on the unit circle when phase_only,
    solvers.py:280-282), the gain weights as given, iteration count 1, and
    the residual of those gains."""
    c = _ragged(65, 2, 1, 2, seed=3100)
    rng = np.random.default_rng(5)
    shape = (2, 65, 2, 1, 1)
    gain0 = rng.uniform(0.8, 1.2, shape) * np.exp(1j * rng.uniform(-1, 1, shape))
    gwt0 = rng.uniform(0.5, 1.5, shape)
    got, want = _parity(f"3c/niter0_po{int(phase_only)}", c, 0, 0, phase_only=phase_only,
                        gain0=gain0, gwt0=gwt0)
    assert np.all(got[3] == 1)
    np.testing.assert_allclose(got[0], gain0 / np.abs(gain0) if phase_only else gain0, rtol=1e-14)
    np.testing.assert_array_equal(got[1], gwt0)


@pytest.mark.parametrize("kw", [dict(refant=100), dict(refant=7), dict(damping=0.0),
                                dict(damping=0.25), dict(damping=0.9)],
                         ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()))
def test_refant_and_damping(kw):
    """130 antennas: the reference antenna in the second column block, the
    reference antenna without baselines (its new gain is 0 and numpy.angle(0)
    = 0: no rotation), and dampings other than 0.5."""
    c = _ragged(130, 2, 1, 2, seed=4000)
    assert c["lonely"] == 7
    got, want = _parity("3d/" + "_".join(f"{k}{v}" for k, v in kw.items()), c, 0, 6, **kw)
    if kw.get("refant") == 100:
        assert np.max(np.abs(got[0][:, 100].imag)) < 1e-6 and np.max(np.abs(want[0][:, 0].imag)) > 1e-2


@pytest.mark.parametrize("mode,npol,nchan", [(0, 1, 63), (0, 1, 64), (0, 1, 65),
                                             (1, 4, 15), (1, 4, 16), (1, 4, 17)])
def test_fill_tile_switch(mode, npol, nchan):
    """k_fill's 32-wide tile below 64 (chan, comp) columns and the 64-wide one
    from there up: 63 / 64 / 65 columns in scalar mode, 60 / 64 / 68 with four
    components, the baseline count no multiple of either tile."""
    c = _ragged(20, nchan, npol, 2, seed=5000 + nchan)
    assert len(c["a1"]) % 32 != 0
    _parity(f"3e/mode{mode}_{nchan}chan", c, mode, 6)


def test_scratch_reuse_small_after_large():
    """37 antennas, then 300, then the first again in one process: the
    scratch buffers keep the larger solve's x, and only the zeroed weights
    keep it out of the smaller one."""
    small = _ragged(37, 2, 1, 2, seed=6037)
    large = _ragged(300, 2, 1, 2, seed=6300)
    first, want = _parity("3f/37_first", small, 0, 6)
    _parity("3f/300", large, 0, 6)
    again, _ = _parity("3f/37_again", small, 0, 6)
    _check("3f/37_again_vs_first", again[:3], first[:3])


def test_refusals():
    """Arguments the ABI refuses before any launch."""
    import torch
    from ska_sdp_func_python_amd import kernels

    def call(nants=8, npol=1, mode=0, refant=0, gain=None):
        nrec = 1 if mode == 0 else 2
        a1, a2 = np.triu_indices(min(nants, 8), 1)
        perm, conj, rs, ant2 = kernels.canonical_baselines(a1, a2, nants)
        xb = torch.ones((1, a1.size, 1, npol), dtype=torch.complex128, device="cuda")
        wb = torch.ones((1, a1.size, 1, npol), dtype=torch.float64, device="cuda")
        if gain is None:
            gain = torch.ones((1, nants, 1, nrec, nrec), dtype=torch.complex128, device="cuda")
        gwt = torch.zeros(gain.shape, dtype=torch.float64, device="cuda")
        return kernels.solve_gains(xb, wb, gain, gwt, rs, ant2, mode=mode, niter=2, tol=0.0,
                                   refant=refant)

    call()  # the accepted form of the calls below
    for bad in (dict(nants=1025), dict(refant=8), dict(mode=1, npol=2), dict(mode=0, npol=4)):
        with pytest.raises(ValueError):
            call(**bad)
    strided = torch.ones((1, 8, 2, 1, 1), dtype=torch.complex128, device="cuda")[:, :, ::2]
    assert not strided.is_contiguous()
    with pytest.raises(ValueError):
        call(gain=strided)
