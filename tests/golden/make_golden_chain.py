"""Generate the chain-calibration fixtures (tests/golden/chain_*.npz,
gaintable_ops.npz) from the REFERENCE's own code.

Run where the reference sources are (they never travel to the GPU box):
    python tests/golden/make_golden_chain.py

As make_golden.py: the function bodies of the reference's
calibration/chain_calibration.py (calibrate_chain, solve_calibrate_chain,
apply_calibration_chain, create_calibration_controls), calibration/
operations.py (apply_gaintable, multiply_gaintables) and calibration/jones.py
(apply_jones) are AST-extracted and executed over the datamodels shim, with
make_golden's solver namespace behind solve_gaintable.  Only inputs and
outputs are stored.  Visibilities are simulated as in make_golden's
_solver_case: a point-source-like model with the true gains of every Jones
term applied, plus noise.  Every reference solve must converge before niter:
a solve that runs out of iterations logs "gain solution failed", and the
generator refuses to store such a case.

Fixtures (tests/chain_cases.py rebuilds the objects from them):
  chain_T_p1         stokesI, "T", phase only, one row per integration
  chain_TG_p1        stokesI, "TG", G complex over three integrations
  chain_TGB_p4       linear, "TGB", 4 channels: T per integration, G over two
                     integrations, B one row x 4 channels
  chain_GB_p2_gated  linearnp, "GB" at iteration 0 with B's first_selfcal 1
  chain_existing     tables given as a GainTable, a list (with a table of a
                     foreign jones_type) and a dict
  chain_solve_nomodel  solve_calibrate_chain with all weights zero, and with
                     model_vis None
  chain_apply_list / _gated / _nomatch   apply_calibration_chain, forward
  gaintable_ops      multiply_gaintables (nrec 1, 2, errors), apply_jones
"""

import json
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
from make_golden import dm, load_reference, save  # noqa: E402

import chain_cases as cc  # noqa: E402


class _Failures(logging.Handler):
    """Collects the reference's "gain solution failed" warnings."""

    def __init__(self):
        super().__init__(logging.WARNING)
        self.seen = []

    def emit(self, record):
        if "failed" in record.getMessage():
            self.seen.append(record.getMessage())


FAILED = _Failures()
logging.getLogger("reference").addHandler(FAILED)


def reference():
    """The reference's chain functions over its own solver and apply."""
    solver = mg._ref_solver_namespace()
    ops = load_reference("calibration/operations.py", ["apply_gaintable", "multiply_gaintables"],
                         {"copy": __import__("copy"), "numpy": np, "Time": None})
    chain = load_reference(
        "calibration/chain_calibration.py",
        ["create_calibration_controls", "apply_calibration_chain", "calibrate_chain",
         "solve_calibrate_chain"],
        {"create_gaintable_from_visibility": dm.create_gaintable_from_visibility,
         "apply_gaintable": ops["apply_gaintable"], "solve_gaintable": solver["solve_gaintable"]})
    jones = load_reference("calibration/jones.py", ["apply_jones"])
    return chain, ops, jones


def simulate(pf, nants, ntimes, nchan, seed, g_slice=None, unit_model=False, noise=1e-4):
    """(vis, model) Visibilities: times 10 s apart; observed = G1 M G2^H with
    diagonal true gains T (a phase per time and antenna) x G (amplitude and
    phase per ``g_slice`` integrations, antenna and receptor) x B (per
    antenna, channel and receptor), plus noise."""
    rng = np.random.default_rng(seed)
    p = dm.PolarisationFrame(pf)
    npol = p.npol
    nrec = 1 if npol == 1 else 2
    a1, a2 = np.triu_indices(nants, 1)
    bl = np.stack([a1, a2], 1)
    shape = (ntimes, len(bl), nchan, npol)
    model = rng.normal(1.0, 0.2, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))
    if unit_model:
        model = np.ones(shape, complex)
    if npol == 4:
        model[..., 1:3] *= 0.1
    t_ph = rng.normal(0, 0.3, (ntimes, nants, 1, 1))
    g_rows = -(-ntimes // (g_slice or ntimes))
    g_amp = rng.lognormal(0, 0.1, (g_rows, nants, 1, nrec))
    g_ph = rng.normal(0, 0.3, (g_rows, nants, 1, nrec))
    b_amp = rng.lognormal(0, 0.05, (1, nants, nchan, nrec))
    b_ph = rng.normal(0, 0.2, (1, nants, nchan, nrec))
    row_of = np.arange(ntimes) // (g_slice or ntimes)
    g = np.exp(1j * t_ph) * (g_amp * np.exp(1j * g_ph))[row_of] * (b_amp * np.exp(1j * b_ph))
    rec1, rec2 = {1: ([0], [0]), 2: ([0, 1], [0, 1]), 4: ([0, 0, 1, 1], [0, 1, 0, 1])}[npol]
    obs = g[:, a1][..., rec1] * model * np.conj(g[:, a2][..., rec2])
    obs = obs + noise * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    times = 100.0 + 10.0 * np.arange(ntimes)
    vis = dm.Visibility.constructor(
        frequency=np.linspace(1.0e8, 1.1e8, nchan), channel_bandwidth=np.full(nchan, 1e6),
        phasecentre=dm.SkyCoord(0.0, -0.8), uvw=np.zeros((ntimes, len(bl), 3)), time=times,
        vis=obs, baselines=bl, polarisation_frame=p, integration_time=np.full(ntimes, 10.0))
    modelvis = vis.copy(deep=True)
    modelvis["vis"].data = model
    return vis, modelvis


def vis_arrays(vis, modelvis, pf):
    return dict(vis=vis["vis"].data.copy(), model=modelvis["vis"].data.copy(),
                vis_weight=vis["weight"].data.copy(), time=np.asarray(vis.time.data),
                integration_time=np.asarray(vis.integration_time.data),
                frequency=np.asarray(vis.frequency.data), baselines=np.asarray(vis.baselines.data),
                pol_frame=np.array(pf))


def table_arrays(prefix, gt):
    return {f"{prefix}_{k}": np.asarray(gt[k].data).copy()
            for k in ("gain", "weight", "residual", "time", "interval", "frequency")}


def settings(context, controls, iteration):
    return dict(context=np.array(context), controls=np.array(json.dumps(controls)),
                iteration=np.array(iteration))


def run_chain(chain, vis, modelvis, context, controls, iteration, gaintables=None, tag=""):
    """calibrate_chain and solve_calibrate_chain of the reference on copies;
    both must have converged."""
    FAILED.seen.clear()
    out = {}
    v = vis.copy(deep=True)
    cvis, gts = chain["calibrate_chain"](v, modelvis, gaintables=cc.copy_tables(gaintables),
                                         calibration_context=context, controls=controls,
                                         iteration=iteration)
    assert cvis is v
    out[f"{tag}cal_letters"] = np.array("".join(gts.keys()))
    out[f"{tag}cal_vis"] = cvis["vis"].data.copy()
    out[f"{tag}cal_weight"] = cvis["weight"].data.copy()
    for c, t in gts.items():
        out.update(table_arrays(f"{tag}cal_{c}", t))
    sol = chain["solve_calibrate_chain"](vis.copy(deep=True), modelvis,
                                         gaintables=cc.copy_tables(gaintables),
                                         calibration_context=context, controls=controls,
                                         iteration=iteration)
    out[f"{tag}sol_letters"] = np.array("".join(sol.keys()))
    for c, t in sol.items():
        out.update(table_arrays(f"{tag}sol_{c}", t))
    assert not FAILED.seen, FAILED.seen
    return out


def make_chains():
    chain, _, _ = reference()
    base = chain["create_calibration_controls"]()   # chain_T_p1 stores it unchanged

    def controls(**kw):
        c = json.loads(json.dumps(base))
        for letter, upd in kw.items():
            c[letter].update(upd)
        return c

    cases = {
        "T_p1": ("stokesI", 8, 4, 2, "T", controls(), 0, None),
        "TG_p1": ("stokesI", 8, 6, 2, "TG", controls(G={"timeslice": 25.0}), 0, 3),
        "TGB_p4": ("linear", 7, 4, 4, "TGB", controls(G={"timeslice": 15.0}), 0, 2),
        "GB_p2_gated": ("linearnp", 7, 4, 3, "GB",
                        controls(G={"timeslice": 15.0}, B={"first_selfcal": 1}), 0, 2),
    }
    for k, (pf, nants, ntimes, nchan, context, ctl, iteration, g_slice) in cases.items():
        vis, modelvis = simulate(pf, nants, ntimes, nchan, seed=len(k) + nants, g_slice=g_slice)
        out = run_chain(chain, vis, modelvis, context, ctl, iteration)
        if k == "GB_p2_gated":
            assert str(out["cal_letters"]) == "G" and str(out["sol_letters"]) == "GB"
            assert np.all(out["sol_B_gain"][..., 0, 0] == 1.0)
        if k == "TGB_p4":
            assert out["cal_T_gain"].shape[0] == 4 and out["cal_G_gain"].shape[0] == 2
            assert out["cal_B_gain"].shape[:3] == (1, nants, 4)
        if k == "TG_p1":
            assert out["cal_G_gain"].shape[0] == 2
        save(f"chain_{k}.npz", **vis_arrays(vis, modelvis, pf), **settings(context, ctl, iteration),
             **out)


def _start_table(vis, jones, timeslice, rng):
    gt = dm.create_gaintable_from_visibility(vis, timeslice=timeslice, jones_type=jones)
    shape = gt["gain"].data.shape
    gt["gain"].data = rng.uniform(0.9, 1.1, shape) * np.exp(1j * rng.uniform(-0.2, 0.2, shape))
    return gt


def make_existing():
    """Starting tables that are not all ones, handed over in the three forms."""
    chain, _, _ = reference()
    ctl = chain["create_calibration_controls"]()
    ctl["G"]["timeslice"] = 25.0
    pf = "stokesI"
    vis, modelvis = simulate(pf, 8, 6, 2, seed=23, g_slice=3)
    rng = np.random.default_rng(5)
    t_in = _start_table(vis, "T", "auto", rng)
    g_in = _start_table(vis, "G", 25.0, rng)
    b_in = _start_table(vis, "B", 1e5, rng)  # foreign to the context "TG"
    out = {}
    for c, t in (("T", t_in), ("G", g_in), ("B", b_in)):
        out.update(table_arrays(f"in_{c}", t))
    forms = {"single": t_in, "list": [g_in, t_in, b_in], "dict": {"T": t_in, "G": g_in}}
    for form, tables in forms.items():
        out.update(run_chain(chain, vis, modelvis, "TG", ctl, 0, gaintables=tables,
                             tag=f"{form}_"))
        assert str(out[f"{form}_cal_letters"]) in ("TG", "GT")
    save("chain_existing.npz", **vis_arrays(vis, modelvis, pf), **settings("TG", ctl, 0), **out)


def make_solve_nomodel():
    chain, _, _ = reference()
    ctl = chain["create_calibration_controls"]()
    ctl["G"]["timeslice"] = 25.0
    pf = "stokesI"
    vis, modelvis = simulate(pf, 8, 6, 2, seed=31, g_slice=3, unit_model=True)
    out = {}
    FAILED.seen.clear()
    zero = vis.copy(deep=True)
    zero["weight"].data[...] = 0.0
    for c, t in chain["solve_calibrate_chain"](zero, modelvis, calibration_context="TG",
                                               controls=ctl).items():
        out.update(table_arrays(f"zerowt_{c}", t))
        assert np.all(t["gain"].data == 1.0)
    for c, t in chain["solve_calibrate_chain"](vis.copy(deep=True), None, calibration_context="TG",
                                               controls=ctl).items():
        out.update(table_arrays(f"nomodel_{c}", t))
        assert not np.all(t["gain"].data == 1.0)
    assert not FAILED.seen, FAILED.seen
    save("chain_solve_nomodel.npz", **vis_arrays(vis, modelvis, pf), **settings("TG", ctl, 0),
         **out)


def make_apply():
    """apply_calibration_chain (forward) on linear 4-pol data, 3 channels:
    T and G have one channel (the reference then corrects channel 0 only)."""
    chain, _, _ = reference()
    pf = "linear"
    vis, modelvis = simulate(pf, 6, 4, 3, seed=41, g_slice=2)
    rng = np.random.default_rng(6)
    vis["weight"].data = rng.uniform(0.5, 2.0, vis["weight"].data.shape)
    tables = {}
    for c, ts in (("T", "auto"), ("G", 15.0)):
        t = dm.create_gaintable_from_visibility(vis, timeslice=ts, jones_type=c)
        shape = t["gain"].data.shape
        t["gain"].data = (rng.normal(1.0, 0.2, shape)
                           * np.exp(1j * rng.uniform(-np.pi, np.pi, shape)))
        tables[c] = t
    common = vis_arrays(vis, modelvis, pf)
    for c, t in tables.items():
        common.update(table_arrays(f"in_{c}", t))
    runs = {"list": ("TG", 0, {}), "gated": ("TG", 1, {"G": {"first_selfcal": 2}}),
            "nomatch": ("B", 0, {})}
    for k, (context, iteration, upd) in runs.items():
        ctl = chain["create_calibration_controls"]()
        for letter, u in upd.items():
            ctl[letter].update(u)
        v = vis.copy(deep=True)
        got = chain["apply_calibration_chain"](v, [tables["G"], tables["T"]],
                                               calibration_context=context, controls=ctl,
                                               iteration=iteration)
        if k == "nomatch":
            assert np.array_equal(got["vis"].data, vis["vis"].data)
        else:
            assert not np.array_equal(got["vis"].data, vis["vis"].data)
        save(f"chain_apply_{k}.npz", **common, **settings(context, ctl, iteration),
             list_order=np.array("GT"), out_vis=got["vis"].data.copy(),
             out_weight=got["weight"].data.copy())


def make_gaintable_ops():
    _, ops, jones = reference()
    rng = np.random.default_rng(8)
    out = {}

    def table(nrec, time, seed):
        r = np.random.default_rng(seed)
        shape = (len(time), 5, 3, nrec, nrec)
        gain = r.normal(size=shape) + 1j * r.normal(size=shape)   # non-symmetric 2x2
        return dm.GainTable.constructor(
            gain, time, np.full(len(time), 10.0), r.uniform(0.5, 2.0, shape),
            r.uniform(0.0, 0.1, (len(time), 3, nrec, nrec)), np.linspace(1e8, 1.1e8, 3),
            dm.PolarisationFrame("stokesI" if nrec == 1 else "linear"))

    time = np.array([100.0, 110.0, 120.0])
    for nrec in (1, 2):
        a, b = table(nrec, time, 10 + nrec), table(nrec, time + 5e-4, 20 + nrec)
        for name, t in (("a", a), ("b", b)):
            out[f"mul{nrec}_{name}_gain"] = t["gain"].data.copy()
            out[f"mul{nrec}_{name}_weight"] = t["weight"].data.copy()
        prod = ops["multiply_gaintables"](a, b)
        assert prod is a
        out[f"mul{nrec}_gain"] = prod["gain"].data.copy()
        out[f"mul{nrec}_weight"] = prod["weight"].data.copy()
    out["mul_time"] = time
    out["mul_time_b"] = time + 5e-4
    for name, a, b in (("time", table(1, time, 1), table(1, time + 0.01, 2)),
                       ("structure", table(1, time, 1), table(2, time, 2))):
        try:
            ops["multiply_gaintables"](a, b)
            raise AssertionError(name)
        except ValueError as e:
            out[f"mul_error_{name}"] = np.array(str(e).split(":")[0].split("<")[0].strip())
    ej = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
    cfs = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
    small = 1e-4 * ej
    out.update(jones_ej=ej, jones_cfs=cfs, jones_small=small,
               jones_forward=jones["apply_jones"](ej, cfs),
               jones_inverse=jones["apply_jones"](ej, cfs, inverse=True),
               jones_below=jones["apply_jones"](small, cfs, inverse=True),
               jones_below_min_det=jones["apply_jones"](small, cfs, inverse=True, min_det=1e-12))
    assert np.all(out["jones_below"] == 0) and not np.all(out["jones_below_min_det"] == 0)
    save("gaintable_ops.npz", **out)


if __name__ == "__main__":
    make_chains()
    make_existing()
    make_solve_nomodel()
    make_apply()
    make_gaintable_ops()
