"""CPU checks of the visibility operations: the numpy restatements
(tests/visops_restatement.py) against the reference's outputs in
tests/golden/visops_*.npz, the Python layer of visibility/operations.py with
the device calls replaced by the restatements, the functions that need no
kernel, and the host-side errors."""

import numpy as np
import pytest
import torch

import visops_restatement as R

STOKES_I_FRAMES = ["linear", "linearnp", "circular", "circularnp"]
CONTINUUM = [("deg0", 0, False), ("deg1", 1, False), ("deg2", 2, False), ("deg1_mask", 1, True)]
FIELDS = ("vis", "weight", "imaging_weight", "flags")


def _inputs(g):
    return g["vis"], g["weight"], g["imaging_weight"], g["flags"]


def _assert_equal(got, g, suffix=""):
    for name, a in zip(FIELDS, got):
        ref = g[f"out_{name}{suffix}"]
        assert a.shape == ref.shape, name
        assert np.array_equal(a, ref), f"{name}{suffix} differs from the reference"


# ---- 1. restatements against the reference ---------------------------------
@pytest.mark.parametrize("frame", ["linear", "stokesI"])
def test_integrate_restatement_is_bit_equal(frame):
    g = R.load(f"integrate_{frame}")
    _assert_equal(R.integrate(*_inputs(g)), g)
    # the spectrum flagged on every channel: flag 1, no weight, vis 0
    assert g["out_flags"][0, 3, 0, 0] == 1 and g["out_weight"][0, 3, 0, 0] == 0
    assert g["out_flags"].sum() == 1


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_average_restatement_is_bit_equal(G):
    g = R.load("average_linear")
    _assert_equal(R.average(*_inputs(g), G), g, f"_G{G}")
    # the flag count of a group is compared with the total nchan (:292)
    assert g[f"out_flags_G{G}"].sum() == (1 if G == 8 else 0)


@pytest.mark.parametrize("frame", ["linear", "circular"])
def test_to_stokes_restatement_is_bit_equal(frame):
    g = R.load(f"to_stokes_{frame}")
    v, fl = R.to_stokes(g["vis"], g["flags"], frame)
    assert np.array_equal(v, g["out_vis"]) and np.array_equal(fl, g["out_flags"])
    assert str(g["out_frame"]) == "stokesIQUV"
    assert np.array_equal(g["out_weight"], g["weight"])


@pytest.mark.parametrize("frame", STOKES_I_FRAMES)
def test_to_stokesI_restatement_is_bit_equal(frame):
    g = R.load(f"to_stokesI_{frame}")
    _assert_equal(R.to_stokesI(*_inputs(g)), g)


def test_polframe_restatement_is_bit_equal():
    g = R.load("polframe_linear")
    _assert_equal(R.stokesI_to_polframe(*_inputs(g), 4), g)


@pytest.mark.parametrize("tag,degree,masked", CONTINUUM)
def test_continuum_restatement_matches_reference(tag, degree, masked):
    g = R.load("continuum_linear")
    mask = g["mask"] if masked else None
    out, live = R.remove_continuum(g["vis"], g["weight"], g["flags"], g["frequency"], degree, mask)
    err = np.abs(out - g[f"out_vis_{tag}"]).max() / np.abs(g["vis"]).max()
    print(f"\ncontinuum restatement {tag}: max error {err:.2e} of max|vis|")
    assert err < 1e-12
    deficient = np.flatnonzero((live.reshape(-1) >= 1) & (live.reshape(-1) <= degree))
    assert np.array_equal(deficient, g[f"deficient_{tag}"])
    assert live.min() >= 1


# ---- 2. the Python layer with the device calls replaced --------------------
def _np(t):
    return t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _fake_average(vis, weight, iw, flags, group, variant):
    a = [_np(t) for t in (vis, weight, iw, flags)]
    out = R.integrate(*a) if variant == 0 else R.average(*a, group)
    return tuple(torch.as_tensor(np.ascontiguousarray(o)) for o in out)


def _fake_to_stokes(vis, flags, matrix):
    v = np.einsum("oi,...i->...o", np.asarray(matrix), vis.numpy())
    f = np.logical_or(flags.numpy()[..., 0], flags.numpy()[..., 3])[..., None]
    vis.copy_(torch.as_tensor(v))
    flags.copy_(torch.as_tensor(np.repeat(f, 4, axis=-1).astype(np.int64)))
    return vis, flags


def _fake_to_stokes_i(vis, weight, iw, flags):
    out = R.to_stokesI(*[_np(t) for t in (vis, weight, iw, flags)])
    return tuple(torch.as_tensor(np.ascontiguousarray(o)) for o in out)


def _fake_continuum(vis, weight, flags, x, degree, mask=None, rank_capacity=None):
    m = None if mask is None else mask.numpy().astype(bool)
    out, live = R.remove_continuum(vis.numpy(), weight.numpy(), flags.numpy(), None, degree, m,
                                   host_route=False, x=x.numpy())
    vis.copy_(torch.as_tensor(out))
    live = live.reshape(-1)
    idx = np.flatnonzero((live >= 1) & (live <= degree))
    return torch.as_tensor(idx.astype(np.int32)), len(idx)


@pytest.fixture
def host_layer(monkeypatch):
    from ska_sdp_func_python_amd import _device, kernels
    monkeypatch.setattr(_device, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(kernels, "vis_average_channels", _fake_average)
    monkeypatch.setattr(kernels, "vis_to_stokes", _fake_to_stokes)
    monkeypatch.setattr(kernels, "vis_to_stokes_i", _fake_to_stokes_i)
    monkeypatch.setattr(kernels, "vis_remove_continuum", _fake_continuum)


def _got(v):
    return tuple(np.asarray(v[k].data) for k in FIELDS)


def test_integrate_host_layer(host_layer):
    from ska_sdp_func_python_amd.visibility import integrate_visibility_by_channel
    g = R.load("integrate_linear")
    vis = R.case_visibility(g)
    out = integrate_visibility_by_channel(vis)
    assert out is not vis and isinstance(out["vis"].data, np.ndarray)
    _assert_equal(_got(out), g)
    assert np.array_equal(out.frequency.data, g["out_frequency"])
    assert np.array_equal(out.channel_bandwidth.data, g["out_channel_bandwidth"])
    assert out.visibility_acc.polarisation_frame.type == "linear"
    assert np.array_equal(vis["vis"].data, g["vis"])


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_average_host_layer(host_layer, G):
    from ska_sdp_func_python_amd.visibility import average_visibility_by_channel
    g = R.load("average_linear")
    lst = average_visibility_by_channel(R.case_visibility(g), G)
    assert isinstance(lst, list) and len(lst) == 8 // G
    for i, v in enumerate(lst):
        assert v.vis.shape == (2, 15, 1, 4)
        for k in FIELDS:
            assert np.array_equal(v[k].data, g[f"out_{k}_G{G}"][:, :, i:i + 1])
        assert np.array_equal(v.frequency.data, g[f"out_frequency_G{G}"][i:i + 1])
        assert np.array_equal(v.channel_bandwidth.data, g[f"out_channel_bandwidth_G{G}"][i:i + 1])


@pytest.mark.parametrize("frame", ["linear", "circular"])
def test_to_stokes_host_layer(host_layer, frame):
    from ska_sdp_func_python_amd.visibility import convert_visibility_to_stokes
    g = R.load(f"to_stokes_{frame}")
    vis = R.case_visibility(g)
    varr, farr = vis["vis"].data, vis["flags"].data
    out = convert_visibility_to_stokes(vis)
    assert out is vis and vis["vis"].data is varr and vis["flags"].data is farr
    assert np.array_equal(varr, g["out_vis"]) and np.array_equal(farr, g["out_flags"])
    assert vis.visibility_acc.polarisation_frame.type == "stokesIQUV"
    # a frame that is neither linear nor circular is returned untouched
    again = convert_visibility_to_stokes(vis)
    assert again is vis and np.array_equal(varr, g["out_vis"])


@pytest.mark.parametrize("frame", STOKES_I_FRAMES)
def test_to_stokesI_host_layer(host_layer, frame):
    from ska_sdp_func_python_amd.visibility import convert_visibility_to_stokesI
    g = R.load(f"to_stokesI_{frame}")
    vis = R.case_visibility(g)
    out = convert_visibility_to_stokesI(vis)
    assert out is not vis and out.visibility_acc.polarisation_frame.type == "stokesI"
    _assert_equal(_got(out), g)
    assert np.array_equal(out.frequency.data, g["frequency"])
    assert convert_visibility_to_stokesI(out) is out
    vis.attrs["_polarisation_frame"] = "stokesIQUV"
    with pytest.raises(NameError):
        convert_visibility_to_stokesI(vis)


@pytest.mark.parametrize("tag,degree,masked", CONTINUUM)
def test_continuum_host_layer(host_layer, tag, degree, masked):
    """The rank-deficient spectra go through numpy.polyfit on the host."""
    from ska_sdp_func_python_amd.visibility import remove_continuum_visibility
    g = R.load("continuum_linear")
    vis = R.case_visibility(g)
    varr = vis["vis"].data
    out = remove_continuum_visibility(vis, degree=degree, mask=g["mask"] if masked else None)
    assert out is vis and vis["vis"].data is varr
    err = np.abs(varr - g[f"out_vis_{tag}"]).max() / np.abs(g["vis"]).max()
    print(f"\ncontinuum host layer {tag}: max error {err:.2e} of max|vis|")
    assert err < 1e-12


# ---- 3. functions without a kernel -----------------------------------------
def test_polframe_matches_reference():
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.visibility import convert_visibility_stokesI_to_polframe
    g = R.load("polframe_linear")
    vis = R.case_visibility(g)
    out = convert_visibility_stokesI_to_polframe(vis, dm.PolarisationFrame("linear"))
    assert out is not vis and out.visibility_acc.polarisation_frame.type == "linear"
    _assert_equal(_got(out), g)
    assert convert_visibility_stokesI_to_polframe(vis, dm.PolarisationFrame("stokesI")) is vis
    tv = R.case_visibility(g, to=torch.as_tensor)
    tout = convert_visibility_stokesI_to_polframe(tv, dm.PolarisationFrame("linear"))
    assert isinstance(tout["vis"].data, torch.Tensor)
    _assert_equal(tuple(tout[k].data.numpy() for k in FIELDS), g)


@pytest.mark.parametrize("to", [None, torch.as_tensor])
def test_subtract_visibility(to):
    from ska_sdp_func_python_amd.visibility import subtract_visibility
    g = R.load("integrate_linear")
    vis, model = R.case_visibility(g, to), R.case_visibility(g, to)
    model["vis"].data = model["vis"].data * 0.25
    res = subtract_visibility(vis, model)
    assert res is not vis and np.array_equal(_np(vis["vis"].data), g["vis"])
    assert np.array_equal(_np(res["vis"].data), g["vis"] - 0.25 * g["vis"])
    assert np.array_equal(_np(res["weight"].data), g["weight"])
    same = subtract_visibility(vis, model, inplace=True)
    assert same is vis and np.array_equal(_np(vis["vis"].data), g["vis"] - 0.25 * g["vis"])


def test_concatenate_frequency_round_trip():
    from ska_sdp_func_python_amd.visibility import (concatenate_visibility,
                                                    concatenate_visibility_frequency)
    g = R.load("integrate_linear")
    vis = R.case_visibility(g)
    parts = []
    for lo, hi in ((0, 3), (3, 8)):
        rep = {k: vis[k].data[:, :, lo:hi] for k in FIELDS}
        rep["frequency"] = g["frequency"][lo:hi]
        rep["channel_bandwidth"] = g["channel_bandwidth"][lo:hi]
        parts.append(vis._copy_with(deep=True, replace=rep))
    for joined in (concatenate_visibility_frequency(parts),
                   concatenate_visibility(parts, dim="frequency")):
        for k in FIELDS:
            assert np.array_equal(joined[k].data, g[k])
        assert np.array_equal(joined.frequency.data, g["frequency"])
        assert np.array_equal(joined.channel_bandwidth.data, g["channel_bandwidth"])
        assert np.array_equal(joined.uvw.data, g["uvw"])
    with pytest.raises(ValueError):
        concatenate_visibility(parts, dim="polarisation")


def test_expand_polarizations():
    from ska_sdp_func_python_amd.visibility import expand_polarizations
    rng = np.random.default_rng(3)
    d4 = rng.normal(size=(3, 5, 4)) + 1j * rng.normal(size=(3, 5, 4))
    assert expand_polarizations(d4) is d4
    assert expand_polarizations(d4, np.complex64).dtype == np.complex64
    d2 = d4[..., :2]
    e2 = expand_polarizations(d2)
    assert np.array_equal(e2[..., 0], d2[..., 0]) and np.array_equal(e2[..., 3], d2[..., 1])
    assert np.all(e2[..., 1:3] == 0)
    e1 = expand_polarizations(d4[..., :1])
    assert np.array_equal(e1[..., 0], d4[..., 0]) and np.array_equal(e1[..., 3], d4[..., 0])
    t2 = expand_polarizations(torch.as_tensor(d2))
    assert isinstance(t2, torch.Tensor) and np.array_equal(t2.numpy(), e2)


def test_nvis_is_the_number_of_time_rows():
    vis = R.case_visibility(R.load("integrate_linear"))
    assert vis.visibility_acc.nvis == 2


# ---- 4. host-side errors (raised before any device is touched) --------------
def test_subtract_shape_mismatch_raises():
    from ska_sdp_func_python_amd.visibility import subtract_visibility
    a = R.case_visibility(R.load("integrate_linear"))
    b = R.case_visibility(R.load("integrate_stokesI"))
    with pytest.raises(AssertionError, match="different shapes"):
        subtract_visibility(a, b)


@pytest.mark.parametrize("G", [None, 3, 0, 16, 2.5])
def test_average_bad_group_raises(G):
    from ska_sdp_func_python_amd.visibility import average_visibility_by_channel
    with pytest.raises(ValueError, match="divide"):
        average_visibility_by_channel(R.case_visibility(R.load("average_linear")), G)


def test_continuum_degree_limit_raises():
    from ska_sdp_func_python_amd.visibility import remove_continuum_visibility
    with pytest.raises(ValueError, match="0 to 5"):
        remove_continuum_visibility(R.case_visibility(R.load("continuum_linear")), degree=6)


def test_continuum_mask_assertion():
    from ska_sdp_func_python_amd.visibility import remove_continuum_visibility
    mask = np.zeros(8, dtype=bool)
    mask[:2] = True
    with pytest.raises(AssertionError, match="Insufficient channels"):
        remove_continuum_visibility(R.case_visibility(R.load("continuum_linear")), degree=1,
                                    mask=mask)


def test_polframe_two_pol_target_raises():
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.visibility import convert_visibility_stokesI_to_polframe
    with pytest.raises(ValueError, match="polarisations"):
        convert_visibility_stokesI_to_polframe(R.case_visibility(R.load("polframe_linear")),
                                               dm.PolarisationFrame("linearnp"))
