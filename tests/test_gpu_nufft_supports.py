"""GPU accuracy of the w-stacking NUFFT at every kernel support: the fp32 path's
W = 2..8 and the fp64 path's W = 9..16 (15 template instantiations of every
gridder and degridder in csrc/wstack.hip), invert and predict, 2-D and
w-stacked, on every bucketing, against the exact direct sums
(oracle/nufft_oracle.py).

The bound is measured, not fixed.  E(prec, W) is the relative RMS error of
oracle/wgrid_cpu (the fp64 / fp32 host restatement of the same algorithm:
same ES kernel beta = 2.30 W, oversampling 2 and plane spacing, so the same
approximation error) against the exact sums on the same inputs, epsilon,
direction and do_wstacking:

  fp64 path (epsilon < 1e-7):  HIP error <= 2 E(double, W) + 3e-13
      (2: the degree-12 edge-tap fit, ~0.15 epsilon per edge tap, DESIGN.md
      "fp64 NUFFT on MFMA"; 3e-13: three one-dimensional tap factors, each
      within the 1e-13 interior bound of tests/test_es_poly_cpu.py)
  fp32 path:                   HIP error <= 2 (E(single, W) + E(single, 8))
      (E(single, 8) is the restatement's own fp32 rounding floor; rounding,
      unlike the approximation error, is not common to two codes that sum in
      different orders)

Every case prints "sweep ..." with the HIP error, E and their ratio;
profiles/nufft_support_sweep.txt is that table from an MI355X run."""

import functools

import numpy as np
import pytest
import torch

import nufft_oracle as orc
from conftest import rel_rms

pytestmark = pytest.mark.gpu
FLIP_UW = np.array([-1.0, 1.0, -1.0])

# epsilon = 1e-1 .. 1e-15 -> W = 2 .. 16, and two values between decades
EPS_DECADES = [float(f"1e-{k}") for k in range(1, 16)]
EPS_SWEEP = EPS_DECADES + [3e-4, 2e-13]
EPS32 = [e for e in EPS_SWEEP if e >= 1e-7]
EPS64 = [e for e in EPS_SWEEP if e < 1e-7]


def T(a, dt=None):
    return torch.as_tensor(np.asarray(a), device=torch.device("cuda:0"), dtype=dt)


# the documented rule W = ceil(-log10(epsilon / 10)), clamped to [2, 8] at or
# above epsilon 1e-7 and to [9, 16] below, written out for the epsilons used
SUPPORT = {**{e: k + 2 for k, e in enumerate(EPS_DECADES)}, 3e-4: 5, 2e-13: 14, 1.0: 2, 1e-18: 16}


# --------------------------------------------------------------------------
# input sets: dict(uvw, freq, ms, wgt, img, npx, npy, px, py)
# --------------------------------------------------------------------------
def _set_random():
    """The generator of tests/test_gpu_nufft_f64.py::_problem (400 rows, 3
    channels, u and v within 0.45 of Nyquist, image 64 x 48, pixsize_y = 0.9
    pixsize_x) with w drawn from 30 times the u, v range: 10 distinct first
    planes at every support (nplanes 11 at W = 2 to 25 at W = 16), not the
    single one of the small tests."""
    rng = np.random.default_rng(171)
    nrow, nchan, umax, frac = 400, 3, 2000.0, 0.45
    freq = np.linspace(1.0e9, 1.2e9, nchan)
    uvw = rng.uniform(-1, 1, (nrow, 3)) * umax * orc.C_LIGHT / freq.max()
    uvw[:, 2] *= 30.0
    ms = rng.normal(size=(nrow, nchan)) + 1j * rng.normal(size=(nrow, nchan))
    wgt = rng.uniform(0.5, 1.5, (nrow, nchan))
    cell = frac / umax
    img = np.random.default_rng(172).normal(size=(64, 48))
    return dict(uvw=uvw, freq=freq, ms=ms, wgt=wgt, img=img, npx=64, npy=48, px=cell,
                py=cell * 0.9)


def _set_taps():
    """Tap boundaries: every u and v exactly on a grid cell centre or exactly
    half-way between two, where the first or last tap falls on |x| = 1 (the
    clamp and zero-select of es_tap, the non-analytic edge of the fp64
    polynomials).  One channel at freq = c, image 64 x 64, pixsize 2^-13: the
    grid coordinate u pixsize ngrid is u / 64 exactly on the 128-cell grid, so
    u, v = 32 k for integers k in [-110, 110]; w random over about ten plane
    spacings; row 0 at the uv origin."""
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(173)
    nrow, npix, pix = 400, 64, 2.0 ** -13
    lay = kernels.wstack_layout([0.0, 1.0, 1.0, 1.0, orc.C_LIGHT, orc.C_LIGHT], npix, npix, pix,
                                pix, 1e-7, True)
    ngx, ngy = lay["ngrid_x"], lay["ngrid_y"]
    assert (ngx, ngy) == (128, 128)
    k = rng.integers(-110, 111, (nrow, 2))
    k[0] = 0
    k[1], k[2] = (110, -110), (-109, 109)  # both extremes, integer and half-integer cells
    uvw = np.empty((nrow, 3))
    uvw[:, 0] = k[:, 0] * (0.5 / (pix * ngx))
    uvw[:, 1] = k[:, 1] * (0.5 / (pix * ngy))
    assert np.all(uvw[:, :2] * pix * ngx * 2 == k)  # exact
    uvw[:, 2] = rng.uniform(-5.0, 5.0, nrow) * lay["dw"]
    ms = rng.normal(size=(nrow, 1)) + 1j * rng.normal(size=(nrow, 1))
    wgt = rng.uniform(0.5, 1.5, (nrow, 1))
    img = rng.normal(size=(npix, npix))
    return dict(uvw=uvw, freq=np.array([orc.C_LIGHT]), ms=ms, wgt=wgt, img=img, npx=npix,
                npy=npix, px=pix, py=pix)


def _set_same_w(nrow):
    """Degenerate w range: `nrow` rows of the random set's geometry that all
    share one w, a single channel: wmin == wmax, nplanes == W, one first
    plane."""
    base = _set_random()
    rng = np.random.default_rng(174 + nrow)
    uvw = base["uvw"][:nrow].copy()
    uvw[:, 2] = 0.37 * np.abs(base["uvw"][:, 2]).max()
    ms = rng.normal(size=(nrow, 1)) + 1j * rng.normal(size=(nrow, 1))
    wgt = rng.uniform(0.5, 1.5, (nrow, 1))
    return dict(base, uvw=uvw, freq=base["freq"][1:2].copy(), ms=ms, wgt=wgt)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return {"random": _set_random, "taps": _set_taps, "one_row": lambda: _set_same_w(1),
            "same_w": lambda: _set_same_w(50)}[name]()


@functools.lru_cache(maxsize=None)
def _exact(name, direction, dow):
    """The exact direct sums of an input set (flip_uw applied), computed once."""
    s = _inputs(name)
    if direction == "invert":
        ex = orc.ms2dirty_exact(s["uvw"] * FLIP_UW, s["freq"], s["ms"], s["wgt"], s["npx"],
                                s["npy"], s["px"], s["py"], dow)
    else:
        ex = orc.dirty2ms_exact(s["uvw"] * FLIP_UW, s["freq"], s["img"], s["wgt"], s["px"],
                                s["py"], dow)
    ex.setflags(write=False)
    return ex


@functools.lru_cache(maxsize=None)
def _restatement(name, direction, dow, prec, eps):
    """(E, support, nplanes) of oracle/wgrid_cpu on an input set: its relative
    RMS error against the exact sums, once per (set, direction, mode,
    precision, epsilon)."""
    import wgrid_cpu
    s = _inputs(name)
    info = {}
    if direction == "invert":
        out, _, _ = wgrid_cpu.ms2dirty(s["uvw"] * FLIP_UW, s["freq"], s["ms"], s["wgt"], s["npx"],
                                       s["npy"], s["px"], s["py"], eps, dow, nthreads=4,
                                       precision=prec, info=info)
    else:
        out, _, _ = wgrid_cpu.dirty2ms(s["uvw"] * FLIP_UW, s["freq"], s["img"], s["wgt"], s["px"],
                                       s["py"], eps, dow, nthreads=4, precision=prec, info=info)
    return rel_rms(out, _exact(name, direction, dow)), info["support"], info["nplanes"]


def bound(name, direction, dow, eps):
    """(bound, E, support the restatement reports): see the module docstring."""
    if eps < 1e-7:
        E, W, _ = _restatement(name, direction, dow, "double", eps)
        return 2.0 * E + 3e-13, E, W
    E, W, _ = _restatement(name, direction, dow, "single", eps)
    E8, W8, _ = _restatement(name, direction, dow, "single", 1e-7)
    assert W8 == 8
    return 2.0 * (E + E8), E, W


def _hip(name, direction, dow, eps):
    """The HIP call (flip_uw, complex128 visibilities both ways): its error
    against the exact sums and the info."""
    from ska_sdp_func_python_amd import kernels
    s = _inputs(name)
    if direction == "invert":
        out, info = kernels.ms2dirty(T(s["uvw"]), T(s["freq"]), T(s["ms"]), T(s["wgt"]), s["npx"],
                                     s["npy"], s["px"], s["py"], eps, dow, flip_uw=True)
    else:
        out, info = kernels.dirty2ms(T(s["uvw"]), T(s["freq"]), T(s["img"]), T(s["wgt"]), s["px"],
                                     s["py"], eps, dow, flip_uw=True, vis_dtype=torch.complex128)
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got))
    return rel_rms(got, _exact(name, direction, dow)), info


def _check(name, direction, dow, eps, path):
    """One case: run, print the table line, assert plan and bound."""
    e, info = _hip(name, direction, dow, eps)
    b, E, W = bound(name, direction, dow, eps)
    print(f"\nsweep {name:8s} {direction:7s} w {int(dow)} eps {eps:.0e} W {info['support']:2d} "
          f"{path:12s} folded {info['folded']} planes {info['nplanes']:2d}: HIP {e:.2e}  "
          f"E {E:.2e}  ratio {e / E:5.2f}  bound {b:.2e}")
    assert info["support"] == W == SUPPORT[eps]
    assert info["fp64"] == (1 if eps < 1e-7 else 0)
    assert abs(info["beta"] - 2.30 * W) <= 2.0 ** -23 * 2.30 * W  # (held as a float32)
    if dow:
        assert info["nplanes"] >= W
    else:
        assert info["nplanes"] == 1
    assert e <= b, (e, b)
    return info


@pytest.fixture(params=["fine", "fine1", "coarse"])
def bucket(request, monkeypatch):
    """The fp32 path's bucketings, as in tests/test_gpu_nufft.py: one-cell
    buckets from the two-level LDS-histogram sort (forced for the predict too
    by SDP_HIP_BUCKET2=2), the same buckets from the single-level global
    histogram (SDP_HIP_BUCKET2=0), and 16x16-cell buckets sub-sorted by cell
    (SDP_HIP_BUCKET=16)."""
    if request.param == "fine":
        monkeypatch.setenv("SDP_HIP_BUCKET2", "2")
    if request.param == "coarse":
        monkeypatch.setenv("SDP_HIP_BUCKET", "16")
    if request.param == "fine1":
        monkeypatch.setenv("SDP_HIP_BUCKET2", "0")
    return request.param


@pytest.fixture(params=["mfma", "single"])
def gridder(request, monkeypatch):
    """The fp64 path's record paths, as in tests/test_gpu_nufft_f64.py: the
    two-level sort's 48-byte records on the MFMA kernels (default), and the
    single-level bucketing (SDP_HIP_BUCKET2=0): VisRec64 records, the VALU
    gridder and the MFMA degridder.  (16-cell buckets are refused there.)"""
    if request.param == "single":
        monkeypatch.setenv("SDP_HIP_BUCKET2", "0")
    return request.param


@pytest.mark.parametrize("eps", EPS32)
@pytest.mark.parametrize("dow", [False, True])
@pytest.mark.parametrize("direction", ["invert", "predict"])
def test_fp32_supports_match_exact(direction, dow, eps, bucket):
    info = _check("random", direction, dow, eps, bucket)
    inv = direction == "invert"
    assert info["bucket"] == (16 if bucket == "coarse" else 1)
    assert info["tiled"] == (1 if bucket == "fine" else 0)
    # invert: k_grid_mfma_pad on 4-padded cells; the degridders' cells are plain
    assert info["padded"] == (1 if inv else 0)
    assert info["folded"] == (1 if inv else 0)
    if dow:
        assert info["nplanes"] - info["support"] + 1 >= 6


@pytest.mark.parametrize("eps", EPS64)
@pytest.mark.parametrize("dow", [False, True])
@pytest.mark.parametrize("direction", ["invert", "predict"])
def test_fp64_supports_match_exact(direction, dow, eps, gridder):
    info = _check("random", direction, dow, eps, gridder)
    inv = direction == "invert"
    assert info["bucket"] == 1
    assert info["tiled"] == (1 if gridder == "mfma" else 0)
    assert info["padded"] == (1 if inv and gridder == "mfma" else 0)
    assert info["folded"] == (1 if inv else 0)
    if dow:
        assert info["nplanes"] - info["support"] + 1 >= 6


@pytest.mark.parametrize("eps", EPS_SWEEP)
@pytest.mark.parametrize("dow", [False, True])
def test_unfolded_invert_supports_match_exact(dow, eps, monkeypatch):
    """The invert without the Hermitian fold (SDP_HIP_HFOLD=0): the full row
    band, the same bound."""
    monkeypatch.setenv("SDP_HIP_HFOLD", "0")
    info = _check("random", "invert", dow, eps, "hfold=0")
    assert info["folded"] == 0 and info["padded"] == 1


@pytest.mark.parametrize("eps", EPS_SWEEP)
@pytest.mark.parametrize("direction", ["invert", "predict"])
def test_tap_boundaries_match_exact(direction, eps):
    """Every u and v on a cell centre or half-way between two (_set_taps)."""
    info = _check("taps", direction, True, eps, "default")
    assert (info["ngrid_x"], info["ngrid_y"]) == (128, 128)
    assert info["nplanes"] - info["support"] + 1 >= 6


@pytest.mark.parametrize("eps", EPS_SWEEP)
@pytest.mark.parametrize("direction", ["invert", "predict"])
@pytest.mark.parametrize("name", ["one_row", "same_w"])
def test_degenerate_w_range_matches_exact(name, direction, eps):
    """One row, and 50 rows sharing one w, single channel: wmin == wmax, so
    the layout is W planes with a single first plane."""
    info = _check(name, direction, True, eps, "default")
    assert info["nplanes"] == info["support"]


@pytest.mark.parametrize("eps,W", [(1.0, 2), (1e-18, 16)])
@pytest.mark.parametrize("direction", ["invert", "predict"])
def test_epsilon_outside_the_supports_is_clamped(direction, eps, W):
    """epsilon = 1 and 1e-18 clamp to W = 2 and W = 16 and run within that
    support's bound."""
    info = _check("random", direction, True, eps, "default")
    assert info["support"] == W
