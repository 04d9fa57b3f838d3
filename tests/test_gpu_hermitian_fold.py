"""GPU tests of the invert's Hermitian fold (Geo::fold in csrc/wstack_types.h): a
visibility with u < 0 is gridded at (-u, -v, -w) with its value conjugated,
so the plane passes run over half the row band.  The dirty image is the real
part of the transform, so the result is that of the unfolded call.

Tolerances: TOL = 5e-6 relative RMS against the exact direct sums
(oracle/nufft_oracle.py) on the fp32 path, as tests/test_gpu_nufft.py; 1e-10
at epsilon 1e-12 (W = 13), as tests/test_gpu_nufft_f64.py; 1e-6 between the
folded and the unfolded run of the same call (the bound test_gpu_nufft.py
uses between two paths: the fp32 sums are regrouped); weight sums rtol 1e-12.

The fp64 NUFFT needs one-cell buckets (the library refuses SDP_HIP_BUCKET=16
with epsilon < 1e-7), so at epsilon 1e-12 the bucketings are the two-level
and the single-level one."""

import functools

import numpy as np
import pytest
import torch

import nufft_oracle as orc
from conftest import rel_rms

pytestmark = pytest.mark.gpu
TOL = 5e-6
TOL64 = 1e-10
FLIP_UW = np.array([-1.0, 1.0, -1.0])
NPX, NPY = 64, 48
INFO_KEYS = ("w0", "dw", "nplanes", "support", "nvis_used")
BUCKET_ENV = {"fine": ("SDP_HIP_BUCKET2", "2"), "fine1": ("SDP_HIP_BUCKET2", "0"),
              "coarse": ("SDP_HIP_BUCKET", "16")}


def T(a, dt=None):
    return torch.as_tensor(np.asarray(a), device=torch.device("cuda:0"), dtype=dt)


def _tol(eps):
    return TOL64 if eps < 1e-7 else TOL


@functools.lru_cache(maxsize=None)
def _problem(seed, nrow=300, nchan=3, umax=2000.0, wscale=12.0):
    """Random +-u, +-v, +-w over several w planes.  Rows 0 and 1 have u > 0
    and w = +-max|w|: both signs of the largest |w| stay on rows of either u
    sign, so the folded and the unfolded w range coincide (with and without
    flip_uw) and the fold rule holds by construction.  Cached: the callers
    do not write to the arrays."""
    rng = np.random.default_rng(seed)
    freq = np.linspace(1.0e9, 1.2e9, nchan)
    uvw = rng.uniform(-1, 1, (nrow, 3)) * umax * orc.C_LIGHT / freq.max()
    uvw[:, 2] *= wscale
    wm = np.abs(uvw[:, 2]).max()
    uvw[0] = [0.3 * np.abs(uvw[:, 0]).max(), uvw[0, 1], wm]
    uvw[1] = [0.6 * np.abs(uvw[:, 0]).max(), uvw[1, 1], -wm]
    ms = rng.normal(size=(nrow, nchan)) + 1j * rng.normal(size=(nrow, nchan))
    wgt = rng.uniform(0.5, 1.5, (nrow, nchan)).astype(np.float32)
    return uvw, freq, ms, wgt, 0.45 / umax


def _vis_values(ms, vdt):
    # (the values the GPU reads)
    return ms.astype(np.complex64).astype(np.complex128) if vdt == torch.complex64 else ms


@functools.lru_cache(maxsize=None)
def _exact(seed, dow, flip, c64):
    uvw, freq, ms, wgt, cell = _problem(seed)
    ms = _vis_values(ms, torch.complex64 if c64 else torch.complex128)
    fl = FLIP_UW if flip else np.ones(3)
    ex = orc.ms2dirty_exact(uvw * fl, freq, ms, wgt, NPX, NPY, cell, cell * 0.9, dow)
    return ex


def _invert(seed, dow, flip, vdt, eps):
    from ska_sdp_func_python_amd import kernels
    uvw, freq, ms, wgt, cell = _problem(seed)
    out, info = kernels.ms2dirty(T(uvw), T(freq), T(ms, vdt), T(wgt), NPX, NPY, cell, cell * 0.9,
                                 eps, dow, flip_uw=flip)
    return out.cpu().numpy(), info


PARITY = [(b, e) for e in (1e-7, 1e-12) for b in ("fine", "fine1", "coarse")
          if not (b == "coarse" and e < 1e-7)]


@pytest.mark.parametrize("bucket,eps", PARITY)
@pytest.mark.parametrize("vdt", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("dow", [False, True])
def test_fold_on_matches_exact(dow, flip, vdt, bucket, eps, monkeypatch):
    monkeypatch.setenv(*BUCKET_ENV[bucket])
    uvw, freq, ms, wgt, _ = _problem(11)
    out, info = _invert(11, dow, flip, vdt, eps)
    e = rel_rms(out, _exact(11, dow, flip, vdt == torch.complex64))
    print(f"\nfold on: w {dow} flip {flip} {vdt} {bucket} eps {eps:.0e}: rel RMS {e:.2e}")
    assert info["folded"] == 1
    assert info["fp64"] == (1 if eps < 1e-7 else 0)
    assert info["bucket"] == (16 if bucket == "coarse" else 1)
    assert info["tiled"] == (1 if bucket == "fine" else 0)
    assert info["nvis_used"] == ms.size
    assert e < _tol(eps)


@pytest.mark.parametrize("eps", [1e-7, 1e-12])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("dow", [False, True])
def test_fold_on_against_off(dow, flip, eps, monkeypatch):
    on, ion = _invert(11, dow, flip, torch.complex128, eps)
    with monkeypatch.context() as m:
        m.setenv("SDP_HIP_HFOLD", "0")
        off, ioff = _invert(11, dow, flip, torch.complex128, eps)
    assert ion["folded"] == 1 and ioff["folded"] == 0
    for k in INFO_KEYS:
        assert ion[k] == ioff[k], k
    e = rel_rms(on, off)
    print(f"\nfold on/off: w {dow} flip {flip} eps {eps:.0e}: rel RMS {e:.2e}")
    assert e < 1e-6


def _vis_call(uvw, freq, ms, wgt, cell, eps, flip, shift=None):
    from ska_sdp_func_python_amd import kernels
    sw = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    out, info = kernels.ms2dirty_vis(T(uvw), T(freq), T(ms[:, :, None], torch.complex128), 0,
                                     T(wgt), None, None, NPX, NPY, cell, cell * 0.9, eps, True,
                                     flip_uw=flip, sumwt=sw, shift_lmn=shift)
    return out.cpu().numpy(), float(sw.cpu()), info


@pytest.mark.parametrize("eps", [1e-7, 1e-12])
@pytest.mark.parametrize("flip", [False, True])
def test_fold_sumwt_and_shift_with_imaginary_vis(flip, eps, monkeypatch):
    """ms2dirty_vis: the weight sum is the unfolded call's; with a non-zero
    shift_lmn and purely imaginary visibilities a conjugate taken before the
    rotation would flip the sign of the folded rows' contribution."""
    uvw, freq, ms, wgt, cell = _problem(11)
    ims = 1j * ms.real
    lmn = (3.0 * cell, -2.0 * cell, -1.0e-5)
    res = {}
    for shift in (None, lmn):
        on = _vis_call(uvw, freq, ims, wgt, cell, eps, flip, shift)
        with monkeypatch.context() as m:
            m.setenv("SDP_HIP_HFOLD", "0")
            off = _vis_call(uvw, freq, ims, wgt, cell, eps, flip, shift)
        assert on[2]["folded"] == 1 and off[2]["folded"] == 0
        for k in INFO_KEYS:
            assert on[2][k] == off[2][k], k
        np.testing.assert_allclose(on[1], off[1], rtol=1e-12)
        np.testing.assert_allclose(on[1], wgt.astype(np.float64).sum(), rtol=1e-12)
        e = rel_rms(on[0], off[0])
        print(f"\nfold on/off vis: flip {flip} eps {eps:.0e} shift {shift is not None}: {e:.2e}")
        assert e < 1e-6
        res[shift is not None] = on[0]
    # against the exact sums: the shift is vis * exp(+2 pi i uvw_lambda . lmn)
    # with the coordinates as given (before flip_uw)
    fl = FLIP_UW if flip else np.ones(3)
    ex0 = orc.ms2dirty_exact(uvw * fl, freq, ims, wgt, NPX, NPY, cell, cell * 0.9, True)
    d = (uvw @ np.asarray(lmn))[:, None] * (freq / orc.C_LIGHT)[None, :]
    ex1 = orc.ms2dirty_exact(uvw * fl, freq, ims * np.exp(2j * np.pi * d), wgt, NPX, NPY, cell,
                             cell * 0.9, True)
    assert rel_rms(res[False], ex0) < _tol(eps)
    assert rel_rms(res[True], ex1) < _tol(eps)


@pytest.mark.parametrize("eps", [1e-7, 1e-12])
def test_rule_says_no(eps, monkeypatch):
    """All w > 0 with both u signs over many planes: the folded w range
    reaches below the unfolded layout's first plane, so the plan stays
    unfolded and is the SDP_HIP_HFOLD=0 plan."""
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(12)
    nrow, nchan, umax = 400, 3, 2000.0
    freq = np.linspace(1.0e9, 1.2e9, nchan)
    uvw = rng.uniform(-1, 1, (nrow, 3)) * umax * orc.C_LIGHT / freq.max()
    uvw[:, 2] = np.abs(uvw[:, 2]) + 1.0
    uvw[:, 2] *= 60
    assert (uvw[:, 0] < 0).any() and (uvw[:, 0] > 0).any()
    ms = rng.normal(size=(nrow, nchan)) + 1j * rng.normal(size=(nrow, nchan))
    wgt = rng.uniform(0.5, 1.5, (nrow, nchan)).astype(np.float32)
    cell = 0.45 / umax
    args = (T(uvw), T(freq), T(ms), T(wgt), NPX, NPY, cell, cell * 0.9, eps, True)
    out, info = kernels.ms2dirty(*args)
    with monkeypatch.context() as m:
        m.setenv("SDP_HIP_HFOLD", "0")
        _, ioff = kernels.ms2dirty(*args)
    assert info["folded"] == 0 and ioff["folded"] == 0
    assert info["nplanes"] > info["support"] + 2  # (many first planes)
    for k in INFO_KEYS + ("nitems", "ngrid_x", "ngrid_y", "bucket", "tiled", "padded"):
        assert info[k] == ioff[k], k
    ex = orc.ms2dirty_exact(uvw, freq, ms, wgt, NPX, NPY, cell, cell * 0.9, True)
    assert rel_rms(out.cpu().numpy(), ex) < _tol(eps)


@pytest.mark.parametrize("bucket,eps", PARITY)
@pytest.mark.parametrize("flip", [False, True])
def test_centre_rows(flip, bucket, eps, monkeypatch):
    """Rows on the fold's edge: u = 0 exactly with v of both signs (not
    folded), u = +-1e-9 m, the origin, and rows at +-max|u|."""
    from ska_sdp_func_python_amd import kernels
    monkeypatch.setenv(*BUCKET_ENV[bucket])
    uvw, freq, ms, wgt, cell = _problem(13, nrow=320)
    uvw = uvw.copy()
    um = np.abs(uvw[:, 0]).max()
    uvw[2:6, 0] = 0.0
    uvw[2:6, 1] = [700.0 * 0.25, -700.0 * 0.25, 31.0, -31.0]
    uvw[6, 0], uvw[7, 0] = 1e-9, -1e-9
    uvw[8] = 0.0
    uvw[9, 0], uvw[10, 0] = um, -um
    ex = orc.ms2dirty_exact(uvw * (FLIP_UW if flip else np.ones(3)), freq, ms, wgt, NPX, NPY, cell,
                            cell * 0.9, True)
    out, info = kernels.ms2dirty(T(uvw), T(freq), T(ms), T(wgt), NPX, NPY, cell, cell * 0.9, eps,
                                 True, flip_uw=flip)
    e = rel_rms(out.cpu().numpy(), ex)
    print(f"\ncentre rows: flip {flip} {bucket} eps {eps:.0e}: rel RMS {e:.2e}")
    assert info["folded"] == 1 and info["nvis_used"] == ms.size
    assert e < _tol(eps)


def _pol_problem(seed):
    rng = np.random.default_rng(seed)
    nrow, nchan, npv, umax = 4000, 6, 4, 3000.0
    freq = np.linspace(1.0e9, 1.2e9, nchan)
    uvw = rng.uniform(-1, 1, (nrow, 3)) * umax * orc.C_LIGHT / freq.max()
    uvw[:, 2] *= 6.0
    wm = np.abs(uvw[:, 2]).max()
    uvw[0, 0], uvw[0, 2] = 100.0, wm
    uvw[1, 0], uvw[1, 2] = 200.0, -wm
    vis = rng.normal(size=(nrow, nchan, npv)) + 1j * rng.normal(size=(nrow, nchan, npv))
    flags = (rng.uniform(size=(nrow, nchan, npv)) < 0.2)
    wgt = rng.uniform(0.5, 2.0, (nrow, nchan, npv))
    wgt[: nrow // 3, :, 0] = 0.0  # pol 0 drops rows the other pols grid
    return uvw, freq, vis, flags, wgt, 0.35 / umax


CONV = [[1, 0, 0, 1], [1, 0, 0, -1], [0, 1, 1, 0], [0, -1j, 1j, 0]]  # linear -> IQUV


def test_pols_call_folded_matches_unfolded_per_pol_calls(monkeypatch):
    """sdp_hip_ms2dirty_vis_pols (one bucketing, one value pass writing
    every pol's records) folded against one unfolded ms2dirty_vis call per
    image pol."""
    from ska_sdp_func_python_amd import kernels
    uvw, freq, vis, flags, wgt, cell = _pol_problem(14)
    uvw_t, freq_t, vis_t = T(uvw), T(freq), T(vis, torch.complex64)
    flags_t, wgt_t = T(flags).to(torch.int8), T(wgt)
    args = (NPX, NPY, cell, cell * 0.9, 1e-7, True)
    ind, sws = [], []
    with monkeypatch.context() as m:
        m.setenv("SDP_HIP_HFOLD", "0")
        for q in range(4):
            sw = torch.zeros(1, dtype=torch.float64, device="cuda:0")
            out, info = kernels.ms2dirty_vis(uvw_t, freq_t, vis_t, q, wgt_t[:, :, q].contiguous(),
                                             flags_t, CONV[q], *args, flip_uw=True, sumwt=sw)
            assert info["folded"] == 0
            ind.append(out.cpu().numpy())
            sws.append(float(sw.cpu()))
    sw4 = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    out4, info = kernels.ms2dirty_vis_pols(uvw_t, freq_t, vis_t, wgt_t, flags_t, CONV, *args,
                                           flip_uw=True, sumwt=sw4)
    assert info["folded"] == 1
    got, gsw = out4.cpu().numpy(), sw4.cpu().numpy()
    for q in range(4):
        e = rel_rms(got[q], ind[q])
        print(f"\npols call folded vs per-pol unfolded, pol {q}: {e:.2e}")
        assert e < 1e-6, q
        np.testing.assert_allclose(gsw[q], sws[q], rtol=1e-12)


@pytest.mark.parametrize("bucket2", ["1", "2"])
def test_kept_bucketing_folded_matches_unfolded_calls(bucket2, monkeypatch):
    """A keep_buckets call and reuse_buckets calls with other weights, folded,
    against independent unfolded calls.  The kept plan carries the fold: a
    reuse call under SDP_HIP_HFOLD=0 still runs (and reports) the kept,
    folded plan."""
    from ska_sdp_func_python_amd import kernels
    monkeypatch.setenv("SDP_HIP_BUCKET2", bucket2)
    uvw, freq, vis, flags, wgt, cell = _pol_problem(15)
    uvw_t, freq_t, vis_t = T(uvw), T(freq), T(vis, torch.complex64)
    flags_t, wgt_t = T(flags).to(torch.int32), T(wgt)
    args = (NPX, NPY, cell, cell * 0.9, 1e-7, True)

    def run(pol, **kw):
        sw = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        out, info = kernels.ms2dirty_vis(uvw_t, freq_t, vis_t, pol, wgt_t[:, :, pol].contiguous(),
                                         flags_t, None, *args, flip_uw=True, sumwt=sw, **kw)
        return out.cpu().numpy(), float(sw.cpu()), info

    with monkeypatch.context() as m:
        m.setenv("SDP_HIP_HFOLD", "0")
        ind = [run(p) for p in range(4)]
    shared = [run(0, keep_buckets=True)] + [run(p, reuse_buckets=True) for p in (1, 2)]
    with monkeypatch.context() as m:
        m.setenv("SDP_HIP_HFOLD", "0")
        shared.append(run(3, reuse_buckets=True))
    for p in range(4):
        assert ind[p][2]["folded"] == 0 and shared[p][2]["folded"] == 1, p
        e = rel_rms(shared[p][0], ind[p][0])
        print(f"\nkept bucketing (BUCKET2={bucket2}) folded vs unfolded, pol {p}: {e:.2e}")
        assert e < 1e-6, p
        np.testing.assert_allclose(shared[p][1], ind[p][1], rtol=1e-12)
    assert shared[0][2]["tiled"] == (1 if bucket2 == "2" else 0)


@pytest.mark.parametrize("eps", [1e-7, 1e-12])
def test_plane_chunked_plan_stays_unfolded(eps, monkeypatch):
    """A plan whose w planes do not all stay resident (a grid budget of one
    plane) is the fall-back of a batch sequence and runs unfolded, as the
    batches do: same layout, parity with the exact sums."""
    _, ion = _invert(11, True, True, torch.complex128, eps)
    with monkeypatch.context() as m:
        m.setenv("SDP_HIP_GRID_BUDGET_GB", "0.000001")
        out, info = _invert(11, True, True, torch.complex128, eps)
    assert ion["folded"] == 1 and ion["grid_launches"] == 1
    assert info["folded"] == 0 and info["grid_launches"] == info["nplanes"] > 1
    for k in INFO_KEYS:
        assert info[k] == ion[k], k
    assert rel_rms(out, _exact(11, True, True, False)) < _tol(eps)
