"""CPU checks of the inverse sky-component DFT: the numpy restatement
(tests/idft_restatement.py) against the reference's outputs in
tests/golden/idft_*.npz, the row-sharded sums over a 2-rank gloo group, and
the return shapes of idft_visibility_skycomponent with the device call
replaced by the restatement."""

import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import golden
from idft_restatement import (idft_case, idft_reference_result, idft_shard_fn, idft_sums,
                              uvw_lambda_of)

CASES = ["linear_iquv", "circular", "stokesI_single"]


def _max_rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_reference(tag):
    g = golden(f"idft_{tag}.npz")
    flux, weights = idft_reference_result(g)
    assert flux.shape == g["flux"].shape and weights.shape == g["weights"].shape
    assert _max_rel(flux, g["flux"]) < 1e-12
    assert _max_rel(weights, g["weights"]) < 1e-12
    # the fully flagged (channel, pol): no weight; in the visibilities' own
    # frame the flux there is exactly 0
    assert np.all(g["weights"][:, 1, -1] == 0)
    if str(g["vis_frame"]) == str(g["comp_frame"]):
        assert np.all(g["flux"][:, 1, -1] == 0) and np.all(flux[:, 1, -1] == 0)


def _shard_problem():
    rng = np.random.default_rng(31)
    nrow, ncomp, npol = 37, 4, 2
    freq = np.array([1.0e9, 1.1e9, 1.3e9])
    uvw = rng.normal(0, 2000, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    shape = (nrow, len(freq), npol)
    vis = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    weight = rng.uniform(0.0, 2.0, shape)
    flags = (rng.uniform(size=shape) < 0.1).astype(np.int64)
    return dc, vis, weight, uvw, freq, flags


def _worker(rank, world, port, data, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ska_sdp_func_python_amd import parallel as par
    T = torch.as_tensor
    dc, vis, weight, uvw, freq, flags = data
    lo, hi = par.shard_range(uvw.shape[0], rank, world)
    dcs = T(dc.copy()) if rank == 0 else torch.zeros_like(T(dc))  # broadcast from 0
    s, w = par.idft_sharded(dcs, T(vis[lo:hi]), T(weight[lo:hi]), T(uvw[lo:hi]), freq=T(freq),
                            flags=T(flags[lo:hi]), idft_fn=idft_shard_fn)
    q.put((rank, s.numpy(), w.numpy()))
    dist.destroy_process_group()


def test_sharded_idft_equals_full():
    data = _shard_problem()
    dc, vis, weight, uvw, freq, flags = data
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + int(np.random.default_rng(31).integers(0, 400))
    procs = [ctx.Process(target=_worker, args=(r, 2, port, data, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    s_full, w_full = idft_sums(dc, vis, weight, uvw_lambda_of(uvw, freq), flags)
    assert len(res) == 2
    for _, s, w in res:
        np.testing.assert_allclose(s, s_full, rtol=1e-12, atol=1e-12 * np.abs(s_full).max())
        np.testing.assert_allclose(w, w_full, rtol=1e-12)


def test_idft_sharded_without_process_group():
    """No process group: the rank's own sums, unchanged."""
    from ska_sdp_func_python_amd import parallel as par
    dc, vis, weight, uvw, freq, flags = _shard_problem()
    T = torch.as_tensor
    s, w = par.idft_sharded(T(dc), T(vis), T(weight), T(uvw), freq=T(freq), flags=T(flags),
                            idft_fn=idft_shard_fn)
    s_full, w_full = idft_sums(dc, vis, weight, uvw_lambda_of(uvw, freq), flags)
    assert np.array_equal(s.numpy(), s_full) and np.array_equal(w.numpy(), w_full)


def test_idft_none_returns_none():
    from ska_sdp_func_python_amd.imaging import idft_visibility_skycomponent
    vis, _, _ = idft_case(golden("idft_stokesI_single.npz"))
    assert idft_visibility_skycomponent(vis, None) is None


@pytest.mark.parametrize("tag", CASES)
def test_idft_return_shapes_host_layer(tag, monkeypatch):
    """The Python layer around the device call (copies, the division, the pol
    conversion, the list shapes; one bare component comes back as a list of
    one) with the device call replaced by the numpy restatement."""
    from ska_sdp_func_python_amd import _device, kernels
    from ska_sdp_func_python_amd.imaging import idft_visibility_skycomponent
    monkeypatch.setattr(_device, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(kernels, "idft_point", idft_shard_fn)
    g = golden(f"idft_{tag}.npz")
    vis, comps, single = idft_case(g)
    before = [c.flux.copy() for c in comps]
    newsc, weights = idft_visibility_skycomponent(vis, comps[0] if single else comps)
    assert isinstance(newsc, list) and isinstance(weights, list)
    assert len(newsc) == len(weights) == len(comps)
    for i, (nc, w) in enumerate(zip(newsc, weights)):
        assert nc is not comps[i] and np.array_equal(comps[i].flux, before[i])
        assert isinstance(nc.flux, np.ndarray) and np.iscomplexobj(nc.flux)
        assert nc.flux.shape == g["flux"][i].shape and w.shape == g["weights"][i].shape
        assert nc.polarisation_frame == comps[i].polarisation_frame
        assert _max_rel(nc.flux, g["flux"][i]) < 1e-12
        assert _max_rel(w, g["weights"][i]) < 1e-12
