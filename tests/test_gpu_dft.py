"""GPU parity of the sky-component DFT (sdp_hip_dft_point_*) against the
reference's dft_cpu_looped outputs (tests/golden/dft_*.npz).
Tolerance: complex128 output (fp64 sincos and sums, the reference's dtype)
|error| RMS / |vis| RMS < 1e-11; complex64 output (fp32 sincos) < 2e-6."""

import numpy as np
import pytest
import torch

from conftest import golden, rel_rms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["p4", "p1_bcast", "p2"])
def test_dft_point_v00_matches_reference(tag):
    from ska_sdp_func_python_amd.imaging.dft import dft_kernel
    g = golden(f"dft_{tag}.npz")
    for name in (None, "cpu_looped", "gpu_cupy_raw", "proc_func", "hip"):
        vis = dft_kernel(g["direction_cosines"], g["vfluxes"], g["uvw_lambda"], name)
        assert rel_rms(vis, g["vis"]) < 1e-11


def test_dft_unknown_kernel_raises():
    from ska_sdp_func_python_amd.imaging.dft import dft_kernel
    g = golden("dft_p4.npz")
    with pytest.raises(ValueError):
        dft_kernel(g["direction_cosines"], g["vfluxes"], g["uvw_lambda"], "nope")


def test_dft_skycomponent_qa_known_answers():
    """reference tests/imaging/test_dft_skycomponent_visibility_kernels.py:33-36."""
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd import simulation
    from ska_sdp_func_python_amd.imaging import dft_skycomponent_visibility
    pc = dm.SkyCoord(180.0, -35.0, unit="deg")
    freq = np.linspace(1.0e8, 1.1e8, 6)
    vis = simulation.make_visibility("LOW", nants=40, ntimes=2, nchan=6, f_lo=1.0e8, f_hi=1.1e8,
                                     polarisation_frame="linear", phasecentre=pc)
    comp = dm.SkyComponent(dm.SkyCoord(181.0, -35.0, unit="deg"), freq,
                           flux=np.array(6 * [100.0, 20.0, -10.0, 1.0]).reshape(6, 4),
                           polarisation_frame=dm.PolarisationFrame("stokesIQUV"))
    res = dft_skycomponent_visibility(vis, 20 * [comp])
    qa = res.visibility_acc.qa_visibility()
    np.testing.assert_almost_equal(qa.data["maxabs"], 2400.0, decimal=3)
    np.testing.assert_almost_equal(qa.data["minabs"], 200.9975124, decimal=3)
    np.testing.assert_almost_equal(qa.data["rms"], 942.9223125, decimal=3)


def test_dft_metres_matches_lambda_form_at_scale():
    """The fused-lambda entry point equals the uvw_lambda one (1e5 vis, 64 comps)."""
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(1)
    dev = torch.device("cuda:0")
    nrow, nchan, ncomp = 20000, 5, 64
    freq = np.linspace(1e9, 1.4e9, nchan)
    uvw = rng.normal(0, 3e4, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    flux = rng.uniform(0.1, 2, (ncomp, 1, 1)).astype(complex)
    uvwl = uvw[:, None, :] * (freq / 299792458.0)[None, :, None]
    a = kernels.dft_point(torch.as_tensor(dc, device=dev), torch.as_tensor(flux, device=dev),
                          torch.as_tensor(uvw, device=dev), freq=torch.as_tensor(freq, device=dev))
    b = kernels.dft_point(torch.as_tensor(dc, device=dev), torch.as_tensor(flux, device=dev),
                          torch.as_tensor(uvwl, device=dev))
    assert rel_rms(a.cpu().numpy(), b.cpu().numpy()) < 1e-6
    # spot-check a few rows against fp64
    ph = np.exp(-2j * np.pi * np.einsum("rfs,cs->rfc", uvwl[:50], dc))
    ref = (ph * flux[:, 0, 0][None, None, :]).sum(-1)
    assert rel_rms(a.cpu().numpy()[:50, :, 0], ref) < 2e-6


def test_dft_c128_output_is_fp64_exact():
    """A complex128 output runs the phase's sincos, the flux and the sums in
    fp64 (the reference's numpy dtype): the direct fp64 sum to 1e-11 (the
    phase reaches 10^3 turns); the complex64 output keeps fp32 sincos
    (< 2e-6)."""
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(2)
    dev = torch.device("cuda:0")
    nrow, nchan, ncomp = 3000, 3, 100
    freq = np.linspace(1e9, 1.4e9, nchan)
    uvw = rng.normal(0, 3e4, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    flux = (rng.uniform(0.1, 2, (ncomp, 1, 2)) + 1j * rng.uniform(-0.1, 0.1, (ncomp, 1, 2)))
    uvwl = uvw[:, None, :] * (freq / 299792458.0)[None, :, None]
    ph = np.exp(-2j * np.pi * np.einsum("rfs,cs->rfc", uvwl, dc))
    ref = np.einsum("rfc,cp->rfp", ph, flux[:, 0, :])
    args = (torch.as_tensor(dc, device=dev), torch.as_tensor(flux, device=dev),
            torch.as_tensor(uvw, device=dev))
    a = kernels.dft_point(*args, freq=torch.as_tensor(freq, device=dev),
                          vis_dtype=torch.complex128)
    b = kernels.dft_point(*args, freq=torch.as_tensor(freq, device=dev))
    assert rel_rms(a.cpu().numpy(), ref) < 1e-11
    assert rel_rms(b.cpu().numpy(), ref) < 2e-6


# k_dft_mfma works in tiles of 16 rows x 16 components; a workgroup covers
# 256 / 128 / 64 rows for npol 1 / 2 / 4 and stages components in chunks of 256.
# (nrow, ncomp): rows below one tile, one short of a tile, one past the
# workgroup of npol 4 and of npol 1; components padded to 16, exactly one chunk
# and a chunk restart with a 1-component tail.  Every nrow and every ncomp
# meets every npol, output type, uvw form and flux layout.
_TILE_EDGES = [(1, 257), (15, 17), (65, 256), (257, 1)]
_SENTINEL = complex(-7.0e30, 3.0e30)
_GUARD_ROWS = 256  # the largest workgroup's rows: what a wrong row guard could reach


def _tile_problem(nrow, ncomp, npol, fnchan):
    """The generator and scales of test_dft_c128_output_is_fp64_exact, 2
    channels, per-channel fluxes that differ when fnchan = 2."""
    rng = np.random.default_rng(1000 * nrow + ncomp)
    freq = np.array([1.0e9, 1.4e9])
    uvw = rng.normal(0, 3e4, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    flux = (rng.uniform(0.1, 2, (ncomp, fnchan, npol)) +
            1j * rng.uniform(-0.1, 0.1, (ncomp, fnchan, npol)))
    uvwl = uvw[:, None, :] * (freq / 299792458.0)[None, :, None]
    ph = np.exp(-2j * np.pi * np.einsum("rfs,cs->rfc", uvwl, dc))
    ref = np.einsum("rfc,cfp->rfp", ph, np.broadcast_to(flux, (ncomp, 2, npol)))
    return dc, flux, uvw, uvwl, freq, ref


@pytest.mark.parametrize("nrow,ncomp", _TILE_EDGES)
@pytest.mark.parametrize("npol", [1, 2, 4])
@pytest.mark.parametrize("vdt", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("metres", [True, False])
@pytest.mark.parametrize("fnchan", [1, 2])
def test_dft_tile_edges(nrow, ncomp, npol, vdt, metres, fnchan):
    """Every k_dft_mfma instantiation (npol 1, 2, 4 x complex64 / complex128
    output x metres / wavelengths) at sizes chosen for their position
    relative to its tiles, against the direct fp64 sum: 1e-11 (complex128) and
    2e-6 (complex64), the file's tolerances.  The output starts as a sentinel:
    every element must be written, and no row past nrow."""
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    dc, flux, uvw, uvwl, freq, ref = _tile_problem(nrow, ncomp, npol, fnchan)
    buf = torch.full((nrow + _GUARD_ROWS, 2, npol), _SENTINEL, dtype=vdt, device=dev)
    t = lambda a: torch.as_tensor(a, device=dev)
    if metres:
        kernels.dft_point(t(dc), t(flux), t(uvw), freq=t(freq), out=buf[:nrow])
    else:
        kernels.dft_point(t(dc), t(flux), t(uvwl), out=buf[:nrow])
    got = buf.cpu().numpy()
    sentinel = np.asarray(_SENTINEL).astype(got.dtype)
    assert np.all(got[nrow:] == sentinel), "rows past nrow were written"
    assert not np.any(got[:nrow] == sentinel), "output elements left unwritten"
    e = rel_rms(got[:nrow], ref)
    print(f"\ndft tile edges nrow {nrow} ncomp {ncomp} npol {npol} {vdt} metres {metres} "
          f"flux chans {fnchan}: rel RMS {e:.2e}")
    assert e < (1e-11 if vdt == torch.complex128 else 2e-6)


@pytest.mark.parametrize("npol", [1, 2, 4])
@pytest.mark.parametrize("vdt", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("metres", [True, False])
def test_dft_no_components_writes_zeros(npol, vdt, metres):
    """ncomp = 0: the output is written as exact zeros (65 rows: one past the
    workgroup of npol 4), and nothing past nrow."""
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    nrow = 65
    _, _, uvw, uvwl, freq, _ = _tile_problem(nrow, 1, npol, 1)
    dc = torch.zeros((0, 3), dtype=torch.float64, device=dev)
    flux = torch.zeros((0, 1, npol), dtype=torch.complex128, device=dev)
    buf = torch.full((nrow + _GUARD_ROWS, 2, npol), _SENTINEL, dtype=vdt, device=dev)
    if metres:
        kernels.dft_point(dc, flux, torch.as_tensor(uvw, device=dev),
                          freq=torch.as_tensor(freq, device=dev), out=buf[:nrow])
    else:
        kernels.dft_point(dc, flux, torch.as_tensor(uvwl, device=dev), out=buf[:nrow])
    got = buf.cpu().numpy()
    assert np.all(got[:nrow] == 0)
    assert np.all(got[nrow:] == np.asarray(_SENTINEL).astype(got.dtype))
