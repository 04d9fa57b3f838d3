"""GPU tests of the visibility operations (csrc/visops.hip through
kernels.vis_* and visibility/operations.py) against the reference's outputs
(tests/golden/visops_*.npz) and the numpy restatements
(tests/visops_restatement.py).

Bounds: complex128 averaging and Stokes results are numpy's bit for bit
(np.array_equal); complex64 input: relative RMS < 2e-7, one fp32 rounding of
the output; the continuum fit: max error < 1e-11 max|vis|, the project's fp64
bound (tests/test_gpu_idft.py)."""

import functools

import numpy as np
import pytest
import torch

import visops_restatement as R
from conftest import rel_rms

pytestmark = pytest.mark.gpu

FIELDS = ("vis", "weight", "imaging_weight", "flags")
STOKES_I_FRAMES = ["linear", "linearnp", "circular", "circularnp"]
CONTINUUM = [("deg0", 0, False), ("deg1", 1, False), ("deg2", 2, False), ("deg1_mask", 1, True)]
C64_RMS = 2e-7
FIT_TOL = 1e-11


def _dev():
    return torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=_dev(), dtype=dtype)


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _case(g, on_device, c64=False):
    def to(a):
        if c64 and np.iscomplexobj(a):
            a = a.astype(np.complex64)
        return _t(a) if on_device else a.copy()
    return R.case_visibility(g, to)


def _check_fields(out, g, suffix="", on_device=False, c64=False, sl=None):
    for k in FIELDS:
        a = out[k].data
        assert isinstance(a, torch.Tensor) == on_device, k
        if on_device:
            assert a.is_cuda
        ref = g[f"out_{k}{suffix}"]
        ref = ref if sl is None else ref[:, :, sl]
        a = _np(a)
        assert a.shape == ref.shape, k
        if k == "vis" and c64:
            assert a.dtype == np.complex64
            e = rel_rms(a, ref)
            print(f"\n  complex64 {k}{suffix}: rel RMS {e:.2e}")
            assert e < C64_RMS
        else:
            assert np.array_equal(a, ref), f"{k}{suffix} differs from the reference"


# ---- 1. golden parity through the public functions --------------------------
@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("frame", ["linear", "stokesI"])
def test_integrate_matches_reference(frame, on_device, c64):
    from ska_sdp_func_python_amd.visibility import integrate_visibility_by_channel
    g = R.load(f"integrate_{frame}")
    vis = _case(g, on_device, c64)
    out = integrate_visibility_by_channel(vis)
    assert out is not vis
    _check_fields(out, g, "", on_device, c64)
    assert np.array_equal(out.frequency.data, g["out_frequency"])
    assert np.array_equal(out.channel_bandwidth.data, g["out_channel_bandwidth"])
    assert out.visibility_acc.polarisation_frame.type == frame
    assert out.vis.shape[2] == 1


@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_average_matches_reference(G, on_device, c64):
    from ska_sdp_func_python_amd.visibility import average_visibility_by_channel
    g = R.load("average_linear")
    vis = _case(g, on_device, c64)
    lst = average_visibility_by_channel(vis, G)
    assert isinstance(lst, list) and len(lst) == 8 // G
    for i, v in enumerate(lst):
        assert v is not vis
        _check_fields(v, g, f"_G{G}", on_device, c64, sl=slice(i, i + 1))
        assert np.array_equal(v.frequency.data, g[f"out_frequency_G{G}"][i:i + 1])
        assert np.array_equal(v.channel_bandwidth.data, g[f"out_channel_bandwidth_G{G}"][i:i + 1])
        assert v.visibility_acc.polarisation_frame.type == "linear"


@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("frame", ["linear", "circular"])
def test_to_stokes_matches_reference(frame, on_device, c64):
    from ska_sdp_func_python_amd.visibility import convert_visibility_to_stokes
    g = R.load(f"to_stokes_{frame}")
    vis = _case(g, on_device, c64)
    varr, farr = vis["vis"].data, vis["flags"].data
    out = convert_visibility_to_stokes(vis)
    assert out is vis and vis["vis"].data is varr and vis["flags"].data is farr
    _check_fields(out, g, "", on_device, c64)
    assert vis.visibility_acc.polarisation_frame.type == "stokesIQUV"
    assert convert_visibility_to_stokes(vis) is vis  # stokesIQUV: untouched
    _check_fields(vis, g, "", on_device, c64)


@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("frame", STOKES_I_FRAMES)
def test_to_stokesI_matches_reference(frame, on_device, c64):
    from ska_sdp_func_python_amd.visibility import convert_visibility_to_stokesI
    g = R.load(f"to_stokesI_{frame}")
    vis = _case(g, on_device, c64)
    out = convert_visibility_to_stokesI(vis)
    assert out is not vis
    _check_fields(out, g, "", on_device, c64)
    assert out.visibility_acc.polarisation_frame.type == "stokesI"
    assert np.array_equal(out.frequency.data, g["frequency"])
    assert np.array_equal(out.channel_bandwidth.data, g["channel_bandwidth"])
    assert convert_visibility_to_stokesI(out) is out


@pytest.mark.parametrize("on_device", [False, True])
def test_polframe_matches_reference(on_device):
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.visibility import convert_visibility_stokesI_to_polframe
    g = R.load("polframe_linear")
    vis = _case(g, on_device)
    out = convert_visibility_stokesI_to_polframe(vis, dm.PolarisationFrame("linear"))
    assert out is not vis and out.visibility_acc.polarisation_frame.type == "linear"
    _check_fields(out, g, "", on_device)


@pytest.mark.parametrize("c64", [False, True])
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("tag,degree,masked", CONTINUUM)
def test_continuum_matches_reference(tag, degree, masked, on_device, c64):
    from ska_sdp_func_python_amd.visibility import remove_continuum_visibility
    g = R.load("continuum_linear")
    vis = _case(g, on_device, c64)
    varr = vis["vis"].data
    out = remove_continuum_visibility(vis, degree=degree, mask=g["mask"] if masked else None)
    assert out is vis and vis["vis"].data is varr
    assert isinstance(varr, torch.Tensor) == on_device
    got, ref = _np(varr), g[f"out_vis_{tag}"]
    if c64:
        e = rel_rms(got, ref)
        print(f"\ncontinuum {tag} complex64: rel RMS {e:.2e}")
        assert got.dtype == np.complex64 and e < C64_RMS
    else:
        e = np.abs(got - ref).max() / np.abs(g["vis"]).max()
        print(f"\ncontinuum {tag}: max error {e:.2e} of max|vis|")
        assert e < FIT_TOL
    for k in ("weight", "flags"):
        assert np.array_equal(_np(vis[k].data), g[k])


# ---- 2. tile edges against the restatement ----------------------------------
# k_average_tiled stages kAvgTile = 512 consecutive elements (a whole number
# of groups of G * npol elements, across row boundaries) per pass, with
# kAvgThreads = 256 lanes each owning output elements; groups of more than 512
# elements go to k_average_long, one workgroup per group, 512 elements per
# pass.  One tile is 512 / npol channels.  (nchan, G): single channels, small
# groups, 64 and 65 (the pairwise sum of npol 1 changes from one leaf to a
# tree above 64 complex numbers and above 128 reals), one channel past a tile
# with G = 1 (more outputs per tile than lanes), two tiles plus one group with
# G = 8 (rows that straddle tiles) and a single group of two tiles plus 3
# channels (k_average_long with a short last pass; for npol 1 the tree in
# global memory).  Rows: 1, and one short of and one past the rows of a tile.
AVG_TILE = 512


def _avg_shapes(npol):
    tile = AVG_TILE // npol
    return [(1, 1), (2, 2), (6, 3), (64, 64), (65, 65), (tile + 1, 1), (2 * tile + 8, 8),
            (2 * tile + 3, 2 * tile + 3)]


def _avg_rows(nchan, npol):
    per_tile = max(1, AVG_TILE // (nchan * npol))
    return sorted({1, max(1, per_tile - 1), per_tile + 1})


def _avg_cases():
    out = []
    for npol in (1, 2, 4):
        for nchan, G in _avg_shapes(npol):
            for rows in _avg_rows(nchan, npol):
                out.append((npol, nchan, G, rows))
    return out


def _run_average(arrs, G, variant, fdt=torch.int64, c64=False):
    from ska_sdp_func_python_amd import kernels
    vis, weight, iw, flags = arrs
    out = kernels.vis_average_channels(_t(vis, torch.complex64 if c64 else torch.complex128),
                                       _t(weight), _t(iw), _t(flags, fdt), G, variant)
    return tuple(o.cpu().numpy() for o in out)


@pytest.mark.parametrize("fdt", [torch.int8, torch.int64])
@pytest.mark.parametrize("npol,nchan,G,rows", _avg_cases())
def test_average_tile_edges(npol, nchan, G, rows, fdt):
    arrs = R.random_case(1, rows, nchan, npol, 7000 + 13 * nchan + npol + rows)
    if nchan > 1:
        arrs[3][0, 0, :, 0] = 1  # one spectrum flagged on every channel
    variants = [(1, R.average(*arrs, G))]
    if G == nchan:
        variants.append((0, R.integrate(*arrs)))
    for variant, ref in variants:
        got = _run_average(arrs, G, variant, fdt)
        for k, a, b in zip(FIELDS, got, ref):
            assert a.shape == b.shape
            assert np.array_equal(a, b), f"variant {variant} {k} differs from numpy"
        got64 = _run_average(arrs, G, variant, fdt, c64=True)
        e = rel_rms(got64[0], ref[0])
        assert got64[0].dtype == np.complex64 and e < C64_RMS, e
        for a, b in zip(got64[1:], ref[1:]):
            assert np.array_equal(a, b)
    if G == nchan and nchan > 1:
        assert ref[3][0, 0, 0, 0] == 1 and ref[1][0, 0, 0, 0] == 0


def test_average_past_one_grid_stride():
    """kAvgMaxBlocks = 4096 workgroups: 4096 * 512 elements + one row, so that
    workgroup 0 strides on to a second tile, which holds the last row."""
    nchan, npol, G = 8, 4, 2
    rows = 4096 * AVG_TILE // (nchan * npol) + 1
    arrs = R.random_case(1, rows, nchan, npol, 99)
    ref = R.average(*arrs, G)
    got = _run_average(arrs, G, 1)
    for k, a, b in zip(FIELDS, got, ref):
        assert np.array_equal(a, b), k


# k_continuum_lds: a workgroup of kContThreads = 256 lanes holds `rows` rows
# in LDS, rows = min(256 / npol, (40 KiB - 8 nchan) / (24 (nchan npol + 4))),
# at least 1; the largest power of two of lanes with rows npol lanes <= 256,
# lanes <= 64 and lanes <= nchan shares each spectrum (their partial sums are
# combined across lanes); at most kContMaxBlocks = 1024 workgroups stride
# over the row chunks; a row above 60 KiB goes to k_continuum_global.  nchan:
# 2 and 5 (many rows per workgroup, one lane per spectrum), 64 (8 lanes), 65
# and 257 (one row per workgroup for npol 4: 64 lanes, with channel counts
# that differ from lane to lane).  Rows: 1 and one past a workgroup's rows;
# for nchan 2 also one past a grid stride (1024 rows-per-workgroup + 1).
def _cont_rows(nchan, npol):
    per_row = (nchan * npol + 4) * 24
    return max(1, min(256 // npol, (40 * 1024 - 8 * nchan) // per_row))


def _cont_cases():
    out = []
    for npol in (1, 4):
        for nchan in (2, 5, 64, 65, 257):
            degrees = [d for d in (0, 1, 2, 3) if d < nchan] + ([5] if nchan == 64 else [])
            for degree in degrees:
                r = _cont_rows(nchan, npol)
                rows = [1, r + 1] + ([1024 * r + 1] if nchan == 2 and degree == 1 else [])
                for nrows in rows:
                    out.append((npol, nchan, degree, nrows))
    return out


def _freq(nchan):
    return np.linspace(1.0e8, 1.2e8, nchan)


def _run_continuum(vis, weight, flags, nchan, degree, mask=None, c64=False):
    from ska_sdp_func_python_amd import kernels
    v = _t(vis, torch.complex64 if c64 else torch.complex128)
    idx, count = kernels.vis_remove_continuum(
        v, _t(weight), _t(flags), _t(R.abscissa(_freq(nchan))), degree,
        mask=None if mask is None else _t(mask))
    return v.cpu().numpy(), idx.cpu().numpy(), count


def _expected_deficient(live, degree):
    live = live.reshape(-1)
    return np.flatnonzero((live >= 1) & (live <= degree))


@pytest.mark.parametrize("npol,nchan,degree,nrows", _cont_cases())
def test_continuum_tile_edges(npol, nchan, degree, nrows):
    """kernels.vis_remove_continuum alone (no host step) against the QR
    restatement: the spectra it fits to 1e-11 max|vis|, the others unchanged
    bit for bit and exactly the rank-deficient ones listed."""
    vis, weight, _, flags = R.random_case(1, nrows, nchan, npol, 8000 + 7 * nchan + npol + degree)
    ref, live = R.remove_continuum(vis, weight, flags, _freq(nchan), degree, host_route=False)
    got, idx, count = _run_continuum(vis, weight, flags, nchan, degree)
    e = np.abs(got - ref).max() / np.abs(vis).max()
    print(f"\ncontinuum nchan {nchan} npol {npol} degree {degree} rows {nrows}: "
          f"max error {e:.2e} of max|vis|, {count} rank deficient")
    assert e < FIT_TOL
    expect = _expected_deficient(live, degree)
    assert count == len(expect) and np.array_equal(idx, expect)
    untouched = np.broadcast_to((live <= degree)[:, :, None, :], vis.shape)
    assert np.array_equal(got[untouched], vis[untouched])
    # complex64: one fp32 rounding of an output no larger than the input; a
    # fitted spectrum can cancel to nothing, so the error is taken against
    # the input's RMS
    got64, idx64, _ = _run_continuum(vis, weight, flags, nchan, degree, c64=True)
    e64 = float(np.sqrt(np.mean(np.abs(got64 - ref) ** 2) / np.mean(np.abs(vis) ** 2)))
    assert got64.dtype == np.complex64 and e64 < C64_RMS, e64
    assert np.array_equal(idx64, expect)


@pytest.mark.parametrize("npol,nchan", [(1, 2600), (4, 700)])
def test_continuum_long_rows(npol, nchan):
    """Rows above 60 KiB of LDS (24 (nchan npol + 4) + 8 nchan bytes) take
    k_continuum_global."""
    assert (nchan * npol + 4) * 24 + 8 * nchan > 60 * 1024
    vis, weight, _, flags = R.random_case(1, 3, nchan, npol, 8100 + npol)
    mask = np.zeros(nchan, dtype=bool)
    mask[10:40] = True
    ref, _ = R.remove_continuum(vis, weight, flags, _freq(nchan), 2, mask, host_route=False)
    got, idx, count = _run_continuum(vis, weight, flags, nchan, 2, mask)
    e = np.abs(got - ref).max() / np.abs(vis).max()
    print(f"\ncontinuum long rows nchan {nchan} npol {npol}: max error {e:.2e} of max|vis|")
    assert e < FIT_TOL and count == 0 and len(idx) == 0


def test_to_stokes_past_one_grid_stride():
    """k_to_stokes_*: 256 lanes, one sample each, at most 4096 workgroups."""
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd import kernels
    nsamp = 4096 * 256 + 1
    vis, weight, iw, flags = R.random_case(1, 1, nsamp, 4, 17)
    m = dm.pol_conversion_matrix(dm.PolarisationFrame("circular"), dm.PolarisationFrame("stokesIQUV"))
    ref_i = R.to_stokesI(vis, weight, iw, flags)
    got_i = kernels.vis_to_stokes_i(_t(vis), _t(weight), _t(iw), _t(flags, torch.int8))
    for k, a, b in zip(FIELDS, got_i, ref_i):
        assert np.array_equal(a.cpu().numpy(), b), k
    ref_v, ref_f = R.to_stokes(vis, flags, "circular")
    v, f = _t(vis), _t(flags, torch.int32)
    kernels.vis_to_stokes(v, f, m)
    assert np.array_equal(v.cpu().numpy(), ref_v) and np.array_equal(f.cpu().numpy(), ref_f)


# ---- 3. the rank route -------------------------------------------------------
def test_continuum_rank_route():
    """Exactly three spectra with 1 <= n_live <= degree and two with n_live = 0.
    Through kernels.vis_remove_continuum alone, without the host step: the
    device list holds exactly those three, all five are unchanged bit for
    bit, and every other spectrum agrees with the restatement -- the host
    fallback's share is this constructed count, not a tolerance."""
    from ska_sdp_func_python_amd.visibility import remove_continuum_visibility
    nbl, nchan, npol, degree = 6, 16, 4, 3
    vis, weight, _, flags = R.random_case(1, nbl, nchan, npol, 31, flag_fraction=0.1)
    assert ((1 - flags).sum(axis=2) > degree).all()
    short = {(0, 1): [4], (2, 3): [0, 15], (5, 2): [3, 8, 9]}   # (baseline, pol): live channels
    empty = [(1, 0), (4, 3)]
    for (b, p), chans in short.items():
        flags[0, b, :, p] = 1
        flags[0, b, chans, p] = 0
    weight[0, 1, :, 0] = 0.0        # no weight ...
    flags[0, 4, :, 3] = 1           # ... and all flagged
    expect = np.array(sorted(b * npol + p for b, p in short))
    ref, live = R.remove_continuum(vis, weight, flags, _freq(nchan), degree, host_route=False)
    assert np.array_equal(_expected_deficient(live, degree), expect)
    assert sorted(np.flatnonzero(live.reshape(-1) == 0)) == sorted(b * npol + p for b, p in empty)
    got, idx, count = _run_continuum(vis, weight, flags, nchan, degree)
    assert count == 3 and np.array_equal(idx, expect)
    for b, p in list(short) + empty:
        assert np.array_equal(got[0, b, :, p], vis[0, b, :, p])
    e = np.abs(got - ref).max() / np.abs(vis).max()
    print(f"\nrank route: kernel alone, max error {e:.2e} of max|vis|")
    assert e < FIT_TOL
    # the public function adds numpy.polyfit's minimum-norm solution for the three
    full, _ = R.remove_continuum(vis, weight, flags, _freq(nchan), degree, host_route=True)
    v = R.case_visibility(dict(vis=vis, weight=weight, imaging_weight=weight, flags=flags,
                               frequency=_freq(nchan), channel_bandwidth=np.full(nchan, 1e6),
                               uvw=np.zeros((1, nbl, 3)), time=np.zeros(1),
                               integration_time=np.ones(1),
                               baselines=np.stack(np.triu_indices(4, 1), 1), frame="linear"), _t)
    remove_continuum_visibility(v, degree=degree)
    e = np.abs(v["vis"].data.cpu().numpy() - full).max() / np.abs(vis).max()
    print(f"rank route: with the host step, max error {e:.2e} of max|vis|")
    assert e < FIT_TOL
    for b, p in empty:
        assert np.array_equal(v["vis"].data.cpu().numpy()[0, b, :, p], vis[0, b, :, p])


# ---- 4. determinism ----------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _det_case():
    return R.random_case(3, 50, 24, 4, 41)


def test_two_runs_are_bit_equal():
    from ska_sdp_func_python_amd import kernels
    vis, weight, iw, flags = _det_case()
    a = _run_average((vis, weight, iw, flags), 4, 1)
    b = _run_average((vis, weight, iw, flags), 4, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    s1 = kernels.vis_to_stokes_i(_t(vis), _t(weight), _t(iw), _t(flags))
    s2 = kernels.vis_to_stokes_i(_t(vis), _t(weight), _t(iw), _t(flags))
    assert all(torch.equal(x, y) for x, y in zip(s1, s2))
    c1, i1, _ = _run_continuum(vis, weight, flags, 24, 2)
    c2, i2, _ = _run_continuum(vis, weight, flags, 24, 2)
    assert np.array_equal(c1, c2) and np.array_equal(i1, i2)


def test_average_rows_split_into_two_calls():
    vis, weight, iw, flags = _det_case()
    whole = _run_average((vis, weight, iw, flags), 4, 1)
    parts = [_run_average(tuple(a[:, lo:hi] for a in (vis, weight, iw, flags)), 4, 1)
             for lo, hi in ((0, 17), (17, 50))]
    for k, w, p0, p1 in zip(FIELDS, whole, *parts):
        assert np.array_equal(w, np.concatenate([p0, p1], axis=1)), k


def test_continuum_rows_split_into_two_calls():
    vis, weight, _, flags = _det_case()
    whole, _, _ = _run_continuum(vis, weight, flags, 24, 2)
    parts = [_run_continuum(vis[:, lo:hi], weight[:, lo:hi], flags[:, lo:hi], 24, 2)[0]
             for lo, hi in ((0, 17), (17, 50))]
    assert np.array_equal(whole, np.concatenate(parts, axis=1))


# ---- 5. subtract_visibility --------------------------------------------------
def test_subtract_visibility_on_device():
    """The major cycle's residual vis - predict on device tensors."""
    from ska_sdp_func_python_amd.visibility import subtract_visibility
    g = R.load("integrate_linear")
    vis, model = _case(g, True), _case(g, True)
    rng = np.random.default_rng(5)
    pred = rng.normal(size=g["vis"].shape) + 1j * rng.normal(size=g["vis"].shape)
    model["vis"].data = _t(pred)
    res = subtract_visibility(vis, model)
    assert res is not vis and res["vis"].data.is_cuda
    assert np.array_equal(res["vis"].data.cpu().numpy(), g["vis"] - pred)
    assert np.array_equal(vis["vis"].data.cpu().numpy(), g["vis"])
    assert np.array_equal(res["flags"].data.cpu().numpy(), g["flags"])
    same = subtract_visibility(vis, model, inplace=True)
    assert same is vis and vis["vis"].data.is_cuda
    assert np.array_equal(vis["vis"].data.cpu().numpy(), g["vis"] - pred)


def test_bad_arguments_raise():
    from ska_sdp_func_python_amd import kernels
    vis, weight, iw, flags = R.random_case(1, 2, 6, 4, 3)
    with pytest.raises(ValueError, match="divide"):
        kernels.vis_average_channels(_t(vis), _t(weight), _t(iw), _t(flags), 4, 1)
    with pytest.raises(ValueError, match="0 to 5"):
        kernels.vis_remove_continuum(_t(vis), _t(weight), _t(flags), _t(R.abscissa(_freq(6))), 6)
    with pytest.raises(ValueError, match="npol"):
        kernels.vis_average_channels(_t(vis[..., :3]), _t(weight[..., :3]), _t(iw[..., :3]),
                                     _t(flags[..., :3]), 2, 1)
