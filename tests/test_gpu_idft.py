"""GPU tests of the inverse sky-component DFT (sdp_hip_idft_point_*,
kernels.idft_point, imaging.idft_visibility_skycomponent) against the
reference's outputs (tests/golden/idft_*.npz) and the direct fp64 numpy sums
(tests/idft_restatement.py).
Tolerances are the forward kernel's (tests/test_gpu_dft.py): |error| RMS /
|sum| RMS < 1e-11 for complex128 visibilities (fp64 sincos, products and
sums), < 2e-6 for complex64 (fp32 sincos and products, sums in fp64 over fp32
partials of at most 32 terms)."""

import functools

import numpy as np
import pytest
import torch

from conftest import golden, rel_rms
from idft_restatement import idft_case, idft_sums, uvw_lambda_of

pytestmark = pytest.mark.gpu

CASES = ["linear_iquv", "circular", "stokesI_single"]


def _t(a):
    return torch.as_tensor(a, device=torch.device("cuda:0"))


def _max_rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- 1. golden parity ------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_idft_matches_reference(tag):
    from ska_sdp_func_python_amd.imaging import idft_visibility_skycomponent
    g = golden(f"idft_{tag}.npz")
    vis, comps, single = idft_case(g)
    newsc, weights = idft_visibility_skycomponent(vis, comps[0] if single else comps)
    assert isinstance(newsc, list) and len(newsc) == len(weights) == len(comps)
    flux = np.array([c.flux for c in newsc])
    w = np.array(weights)
    assert flux.shape == g["flux"].shape and w.shape == g["weights"].shape
    ef, ew = rel_rms(flux, g["flux"]), _max_rel(w, g["weights"])
    print(f"\nidft golden {tag}: flux rel RMS {ef:.2e}, weights max rel {ew:.2e}")
    assert ef < 1e-11
    assert ew < 1e-12
    # the fully flagged (channel, pol) has no weight; where the component is
    # in the visibilities' frame its flux there is exactly 0
    assert np.all(w[:, 1, -1] == 0)
    if str(g["vis_frame"]) == str(g["comp_frame"]):
        assert np.all(flux[:, 1, -1] == 0)
    for c, n in zip(comps, newsc):
        assert n is not c and n.polarisation_frame == c.polarisation_frame


# ---- 2. the reference's round trip (tests/imaging/test_dft_skycomponent_visibility.py:129-157)
@pytest.mark.parametrize("frame", ["linear", "circular", "stokesIQUV"])
def test_idft_returns_the_component(frame):
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd import simulation
    from ska_sdp_func_python_amd.imaging import (dft_skycomponent_visibility,
                                                 idft_visibility_skycomponent)
    pc = dm.SkyCoord(180.0, -35.0, unit="deg")
    vis = simulation.make_visibility("LOW", nants=20, ntimes=2, nchan=6, f_lo=1.0e8, f_hi=1.1e8,
                                     polarisation_frame=frame, phasecentre=pc)
    oned = 100.0 * np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.5])
    comp = dm.SkyComponent(dm.SkyCoord(181.0, -35.0, unit="deg"), vis.frequency.data,
                           flux=np.array([oned] * 4).T, polarisation_frame=dm.PolarisationFrame(frame))
    model = dft_skycomponent_visibility(vis, comp)
    result, _ = idft_visibility_skycomponent(model, comp)
    e = _max_rel(np.real(result[0].flux), comp.flux)
    print(f"\nidft round trip {frame}: max rel {e:.2e}")
    np.testing.assert_allclose(comp.flux, np.real(result[0].flux), rtol=1e-10)


# ---- 3. tile edges ---------------------------------------------------------
# k_idft_mfma stages 256 (complex128) or 512 (complex64) rows per pass (4
# waves x 4 or 8 tiles of 16) against a chunk of 128 / 64 / 32 components for
# npol 1 / 2 / 4.  (nrow, ncomp): the forward test's sizes -- rows below one
# tile, one short of a tile, inside a stage, and 257 (complex128: one past a
# stage, two row partitions' partials are summed) and 513 (the same for
# complex64); components padded to 16, a
# chunk restart with a 1-component tail, whole chunks.  The last size is
# chosen from the launch geometry: with 2 channels and one component chunk
# the rows are cut into at most 2048 / 2 = 1024 partitions, so 1024 * 256 + 1
# rows are 1025 stages in 1024 partitions (complex128) and 513 stages in 512
# partitions (complex64, the count rounded down to a multiple of 8): either
# way many partitions' partials are summed and partition 0 strides on to a
# second stage, which holds the single last row.
_TILE_EDGES = [(1, 257), (15, 17), (65, 256), (257, 1), (513, 3), (1024 * 256 + 1, 1)]
_SENTINEL = complex(-7.0e30, 3.0e30)
_GUARD_COMPS = 128  # the largest component chunk: what a wrong component guard could reach


@functools.lru_cache(maxsize=2)
def _tile_problem(nrow, ncomp, npol):
    """The generator and scales of test_gpu_dft._tile_problem (2 channels, uvw
    sigma 3e4 m, |l|, |m| <= 0.02), random complex visibilities (exactly
    representable in complex64), weights uniform(0, 2) with 10% zeros, 10%
    flags; the fp64 sums without and with the flags."""
    rng = np.random.default_rng(1000 * nrow + ncomp)
    freq = np.array([1.0e9, 1.4e9])
    uvw = rng.normal(0, 3e4, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    shape = (nrow, 2, npol)
    vis = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    weight = rng.uniform(0, 2, shape) * (rng.uniform(size=shape) >= 0.1)
    flags = (rng.uniform(size=shape) < 0.1).astype(np.int32)
    uvwl = uvw_lambda_of(uvw, freq)
    refs = {False: idft_sums(dc, vis, weight, uvwl), True: idft_sums(dc, vis, weight, uvwl, flags)}
    return dc, vis, weight, flags, uvw, uvwl, freq, refs


@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("metres", [True, False])
@pytest.mark.parametrize("vdt", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("npol", [1, 2, 4])
@pytest.mark.parametrize("nrow,ncomp", _TILE_EDGES)
def test_idft_tile_edges(nrow, ncomp, npol, vdt, metres, flagged):
    """Every k_idft_mfma instantiation (npol 1, 2, 4 x complex64 / complex128
    visibilities x metres / wavelengths) with and without flags, at sizes
    chosen for their position relative to its tiles, against the direct fp64
    sums: 1e-11 (complex128) and 2e-6 (complex64); the summed weight to 1e-12.
    The outputs start as a sentinel: every element must be written, and no
    component past ncomp."""
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    dc, vis, weight, flags, uvw, uvwl, freq, refs = _tile_problem(nrow, ncomp, npol)
    ref_s, ref_w = refs[flagged]
    buf = torch.full((ncomp + _GUARD_COMPS, 2, npol), _SENTINEL, dtype=torch.complex128, device=dev)
    wbuf = torch.full((3, npol), _SENTINEL.real, dtype=torch.float64, device=dev)
    kw = dict(flags=_t(flags) if flagged else None, out=(buf[:ncomp], wbuf[:2]))
    if metres:
        kernels.idft_point(_t(dc), _t(vis).to(vdt), _t(weight), _t(uvw), freq=_t(freq), **kw)
    else:
        kernels.idft_point(_t(dc), _t(vis).to(vdt), _t(weight), _t(uvwl), **kw)
    got, gotw = buf.cpu().numpy(), wbuf.cpu().numpy()
    assert np.all(got[ncomp:] == _SENTINEL), "components past ncomp were written"
    assert np.all(gotw[2:] == _SENTINEL.real), "weights past nchan were written"
    assert not np.any(got[:ncomp] == _SENTINEL), "flux_sum elements left unwritten"
    assert not np.any(gotw[:2] == _SENTINEL.real), "sumwt elements left unwritten"
    e, ew = rel_rms(got[:ncomp], ref_s), _max_rel(gotw[:2], ref_w)
    print(f"\nidft tile edges nrow {nrow} ncomp {ncomp} npol {npol} {vdt} metres {metres} "
          f"flags {flagged}: rel RMS {e:.2e}, sumwt max rel {ew:.2e}")
    assert e < (1e-11 if vdt == torch.complex128 else 2e-6)
    assert ew < 1e-12


# ---- 4. accumulation, 5. determinism --------------------------------------
@functools.lru_cache(maxsize=1)
def _long_problem():
    """100000 rows, 5 components, npol 1, complex64: the size at which a
    serial fp32 sum over the rows is at 4.5e-6 to 5.2e-6."""
    rng = np.random.default_rng(5)
    nrow, ncomp = 100000, 5
    freq = np.array([1.2e9])
    uvw = rng.normal(0, 3e4, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    shape = (nrow, 1, 1)
    vis = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    weight = rng.uniform(0, 2, shape)
    ref = idft_sums(dc, vis, weight, uvw_lambda_of(uvw, freq))
    return dc, vis, weight, uvw, freq, ref


def test_idft_accumulation_over_many_rows():
    from ska_sdp_func_python_amd import kernels
    dc, vis, weight, uvw, freq, (ref_s, ref_w) = _long_problem()
    s, w = kernels.idft_point(_t(dc), _t(vis), _t(weight), _t(uvw), freq=_t(freq))
    e, ew = rel_rms(s.cpu().numpy(), ref_s), _max_rel(w.cpu().numpy(), ref_w)
    print(f"\nidft 100000 rows complex64: rel RMS {e:.2e}, sumwt max rel {ew:.2e}")
    assert e < 2e-6
    assert ew < 1e-12


def test_idft_is_deterministic():
    from ska_sdp_func_python_amd import kernels
    dc, vis, weight, uvw, freq, _ = _long_problem()
    args = (_t(dc), _t(vis), _t(weight), _t(uvw))
    s1, w1 = kernels.idft_point(*args, freq=_t(freq))
    s2, w2 = kernels.idft_point(*args, freq=_t(freq))
    same = torch.equal(s1, s2) and torch.equal(w1, w2)
    print(f"\nidft two calls bit-identical: {same}")
    assert torch.equal(s1, s2)
    assert torch.equal(w1, w2)


# ---- 6. adjointness against the forward kernel -----------------------------
def test_idft_is_the_adjoint_of_dft_point():
    """<F, idft(w V)> = <dft(F), w V> in complex128: sum conj(F) S against
    sum w V conj(dft_point(F))."""
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(6)
    nrow, nchan, ncomp, npol = 3000, 2, 100, 2
    freq = np.array([1.0e9, 1.4e9])
    uvw = rng.normal(0, 3e4, (nrow, 3))
    lm = rng.uniform(-0.02, 0.02, (ncomp, 2))
    dc = np.concatenate([lm, (np.sqrt(1 - (lm ** 2).sum(1)) - 1)[:, None]], 1)
    F = rng.normal(size=(ncomp, nchan, npol)) + 1j * rng.normal(size=(ncomp, nchan, npol))
    V = rng.normal(size=(nrow, nchan, npol)) + 1j * rng.normal(size=(nrow, nchan, npol))
    w = rng.uniform(0, 2, (nrow, nchan, npol))
    s, _ = kernels.idft_point(_t(dc), _t(V), _t(w), _t(uvw), freq=_t(freq))
    fwd = kernels.dft_point(_t(dc), _t(F), _t(uvw), freq=_t(freq), vis_dtype=torch.complex128)
    lhs = np.sum(np.conj(F) * s.cpu().numpy())
    rhs = np.sum(w * V * np.conj(fwd.cpu().numpy()))
    e = abs(lhs - rhs) / abs(rhs)
    print(f"\nidft adjointness: |lhs - rhs| / |rhs| {e:.2e}")
    assert e < 1e-11


# ---- 7. degenerate sizes ---------------------------------------------------
@pytest.mark.parametrize("vdt", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("npol", [1, 2, 4])
def test_idft_no_components_writes_only_sumwt(npol, vdt):
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    _, vis, weight, flags, uvw, _, freq, refs = _tile_problem(257, 1, npol)
    dc = torch.zeros((0, 3), dtype=torch.float64, device=dev)
    wbuf = torch.full((3, npol), _SENTINEL.real, dtype=torch.float64, device=dev)
    sbuf = torch.full((_GUARD_COMPS, 2, npol), _SENTINEL, dtype=torch.complex128, device=dev)
    s, w = kernels.idft_point(dc, _t(vis).to(vdt), _t(weight), _t(uvw), freq=_t(freq),
                              flags=_t(flags), out=(sbuf[:0], wbuf[:2]))
    assert tuple(s.shape) == (0, 2, npol)
    assert np.all(sbuf.cpu().numpy() == _SENTINEL), "flux_sum written with no components"
    gotw = wbuf.cpu().numpy()
    ew = _max_rel(gotw[:2], refs[True][1])
    print(f"\nidft ncomp 0 npol {npol} {vdt}: sumwt max rel {ew:.2e}")
    assert ew < 1e-12 and np.all(gotw[2:] == _SENTINEL.real)


@pytest.mark.parametrize("vdt", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("metres", [True, False])
def test_idft_no_rows_writes_zeros(vdt, metres):
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    ncomp, npol = 17, 2
    dc = _tile_problem(15, 17, npol)[0]
    buf = torch.full((ncomp + _GUARD_COMPS, 2, npol), _SENTINEL, dtype=torch.complex128, device=dev)
    wbuf = torch.full((3, npol), _SENTINEL.real, dtype=torch.float64, device=dev)
    vis = torch.zeros((0, 2, npol), dtype=vdt, device=dev)
    weight = torch.zeros((0, 2, npol), dtype=torch.float64, device=dev)
    if metres:
        kernels.idft_point(_t(dc), vis, weight, torch.zeros((0, 3), dtype=torch.float64, device=dev),
                           freq=_t(np.array([1.0e9, 1.4e9])), out=(buf[:ncomp], wbuf[:2]))
    else:
        kernels.idft_point(_t(dc), vis, weight,
                           torch.zeros((0, 2, 3), dtype=torch.float64, device=dev),
                           out=(buf[:ncomp], wbuf[:2]))
    got, gotw = buf.cpu().numpy(), wbuf.cpu().numpy()
    print(f"\nidft nrow 0 {vdt} metres {metres}: max |S| {np.abs(got[:ncomp]).max():.1e}")
    assert np.all(got[:ncomp] == 0) and np.all(gotw[:2] == 0)
    assert np.all(got[ncomp:] == _SENTINEL) and np.all(gotw[2:] == _SENTINEL.real)


def test_idft_bad_npol_raises():
    """npol other than 1, 2, 4: SDP_HIP_ERR_INVALID_ARG, the ValueError that
    the forward path raises."""
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    dc = torch.zeros((2, 3), dtype=torch.float64, device=dev)
    uvw = torch.zeros((4, 3), dtype=torch.float64, device=dev)
    freq = _t(np.array([1.0e9]))
    with pytest.raises(ValueError):
        kernels.dft_point(dc, torch.ones((2, 1, 3), dtype=torch.complex128, device=dev), uvw,
                          freq=freq)
    with pytest.raises(ValueError):
        kernels.idft_point(dc, torch.ones((4, 1, 3), dtype=torch.complex128, device=dev),
                           torch.ones((4, 1, 3), dtype=torch.float64, device=dev), uvw, freq=freq)
    print("\nidft npol 3: ValueError")
