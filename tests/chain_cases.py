"""Objects of the chain-calibration fixtures (tests/golden/chain_*.npz, written
by tests/golden/make_golden_chain.py), rebuilt through the datamodels shim."""

import json

import numpy as np

from ska_sdp_func_python_amd import datamodels as dm

TABLE_VARS = ("gain", "weight", "residual", "time", "interval", "frequency")


def observation(g, device=False, dtype=None):
    """(vis, model) Visibilities of a fixture; ``device``: vis, weight, flags
    and the model as device tensors; ``dtype``: the complex type of both."""
    def build(data):
        nt, nbl = data.shape[:2]
        return dm.Visibility.constructor(
            frequency=g["frequency"], channel_bandwidth=np.full(len(g["frequency"]), 1e6),
            phasecentre=dm.SkyCoord(0.0, -0.8), uvw=np.zeros((nt, nbl, 3)), time=g["time"],
            vis=data.copy(), weight=g["vis_weight"].copy(), baselines=g["baselines"],
            polarisation_frame=dm.PolarisationFrame(str(g["pol_frame"])),
            integration_time=g["integration_time"])

    vis, model = build(g["vis"]), build(g["model"])
    if dtype is not None:
        for v in (vis, model):
            v["vis"].data = v["vis"].data.astype(dtype)
    if device:
        import torch
        for v in (vis, model):
            for k in ("vis", "weight", "flags"):
                v[k].data = torch.as_tensor(v[k].data, device="cuda")
    return vis, model


def settings(g):
    """(context, controls, iteration) of a fixture."""
    return str(g["context"]), json.loads(str(g["controls"])), int(g["iteration"])


def table(g, prefix, jones, vis):
    """The GainTable stored under ``prefix`` (``<prefix>_gain`` ...)."""
    nrec = g[f"{prefix}_gain"].shape[-1]
    pf = vis.visibility_acc.polarisation_frame.type
    rf = "stokesI" if nrec == 1 else ("linear" if pf.startswith("linear") else "circular")
    return dm.GainTable.constructor(
        g[f"{prefix}_gain"].copy(), g[f"{prefix}_time"], g[f"{prefix}_interval"],
        g[f"{prefix}_weight"].copy(), g[f"{prefix}_residual"].copy(), g[f"{prefix}_frequency"],
        dm.PolarisationFrame(rf), vis.phasecentre, None, jones)


def copy_tables(tables):
    """Deep copies of a GainTable, a list or a dict of them (None stays)."""
    if isinstance(tables, dm.GainTable):
        return tables.copy(deep=True)
    if isinstance(tables, list):
        return [t.copy(deep=True) for t in tables]
    if isinstance(tables, dict):
        return {k: t.copy(deep=True) for k, t in tables.items()}
    return tables
