"""Visibility operations (reference src/ska_sdp_func_python/visibility/operations.py).

divide_visibility (:145-189): x = V / M where |M|^2 w > 0 (else 0), weight' =
|M|^2 w -- the point-source equivalent visibility that solve_gaintable
averages; flagged vis, model and weight as the reference's
visibility_acc.flagged_* give them.  One HIP kernel (sdp_hip_divide_vis) with
numpy's complex division.

The streaming operations between the pipeline stages run as one fused HIP
kernel each (csrc/visops.hip): channel averaging (sdp_hip_vis_average_channels),
the Stokes conversions (sdp_hip_vis_to_stokes) and the continuum fit
(sdp_hip_vis_remove_continuum).  Device tensors stay on the device; numpy
input gives numpy output.
"""

import warnings

import numpy as np
import torch

from .. import _device, kernels
from ..datamodels import PolarisationFrame, Visibility, pol_conversion_matrix

_JOIN_VARS = ("vis", "weight", "imaging_weight", "flags")


def _cat(parts, axis):
    if isinstance(parts[0], torch.Tensor):
        return torch.cat([p if isinstance(p, torch.Tensor) else torch.as_tensor(p, device=parts[0].device)
                          for p in parts], dim=axis)
    return np.concatenate([np.asarray(p) for p in parts], axis=axis)


def concatenate_visibility(vis_list, dim="time"):
    """Reference visibility/operations.py:38-72: ``dim="time"`` joins the
    time-dimension arrays, ``dim="frequency"`` the channel axis of vis, weight,
    imaging_weight and flags together with frequency and channel_bandwidth;
    the rest is taken from the first."""
    if not len(vis_list) > 0:
        raise ValueError("concatenate_visibility: vis_list is empty")
    if dim not in ("time", "frequency"):
        raise ValueError(f"concatenate_visibility: dim {dim} is not supported here")
    first = vis_list[0]
    rep = {}
    if dim == "time":
        names, axis = ("vis", "uvw", "weight", "imaging_weight", "flags", "time",
                       "integration_time"), 0
    else:
        names, axis = _JOIN_VARS, 2
        for k in ("frequency", "channel_bandwidth"):
            rep[k] = np.concatenate([np.asarray(v._vars[k]) for v in vis_list])
    for k in names:
        if k not in first._vars:
            continue
        rep[k] = _cat([v._vars[k] for v in vis_list], axis)
    return first._copy_with(deep=True, replace=rep)


def concatenate_visibility_frequency(bvis_list):
    """Reference visibility/operations.py:75-83: the list, in sequence of
    channels, joined along frequency."""
    return concatenate_visibility(bvis_list, "frequency")


def subtract_visibility(vis, model_vis, inplace=False):
    """Reference visibility/operations.py:86-105: vis - model_vis, as a new
    Visibility or (``inplace``) in ``vis``.  Different shapes raise the
    reference's AssertionError."""
    if tuple(vis.vis.shape) != tuple(model_vis.vis.shape):
        raise AssertionError(f"Observed {tuple(vis.vis.shape)} and model visibilities "
                             f"{tuple(model_vis.vis.shape)} have different shapes.")
    v, m = vis["vis"].data, model_vis["vis"].data
    if isinstance(v, torch.Tensor) and not isinstance(m, torch.Tensor):
        m = torch.as_tensor(np.asarray(m), device=v.device)
    elif isinstance(m, torch.Tensor) and not isinstance(v, torch.Tensor):
        m = m.detach().cpu().numpy()
    diff = v - m
    if inplace:
        vis["vis"].data = diff
        return vis
    return vis._copy_with(deep=True, replace={"vis": diff})


def _operands(vis, imaging_weight=True):
    """Contiguous device vis (complex), weight / imaging_weight (f64) and
    flags (an integer type the kernels read) of a Visibility."""
    dev = _device.device()
    v = _device.to_dev(vis["vis"].data, None, dev)
    if v.dtype not in (torch.complex64, torch.complex128):
        v = v.to(torch.complex128)
    w = _device.to_dev(vis["weight"].data, torch.float64, dev).contiguous()
    iw = None
    if imaging_weight:
        iw = _device.to_dev(vis["imaging_weight"].data, torch.float64, dev).contiguous()
    fl = _device.to_dev(vis["flags"].data, None, dev)
    if fl.dtype not in kernels.FLAG_BYTES:
        fl = fl.to(torch.int64)
    return v.contiguous(), w, iw, fl.contiguous()


def _write_back(vis, name, result):
    """In-place semantics: ``result`` (device) into the Visibility's own array
    unless the kernel already worked on it."""
    target = vis[name].data
    if target is result:
        return
    if isinstance(target, torch.Tensor):
        target.copy_(result)
    else:
        target[...] = result.detach().cpu().numpy()


def _like(vis, *arrays):
    """Kernel outputs where the Visibility's own vis lives (device or host)."""
    ref = vis["vis"].data
    return tuple(_device.like_input(a, ref) for a in arrays)


def _new_visibility(vis, v, w, iw, fl, frequency, channel_bandwidth, polarisation_frame):
    out = Visibility.constructor(
        frequency=frequency, channel_bandwidth=channel_bandwidth, phasecentre=vis.phasecentre,
        baselines=vis.baselines.data, configuration=vis.configuration, uvw=vis.uvw.data,
        time=vis.time.data, vis=v, flags=fl, weight=w,
        integration_time=vis.integration_time.data, polarisation_frame=polarisation_frame,
        source=vis.attrs.get("source"), meta=vis.attrs.get("meta"))
    out["imaging_weight"] = iw
    return out


def integrate_visibility_by_channel(vis):
    """Reference visibility/operations.py:192-235: all channels integrated
    into one, as a new Visibility.  flag = 1 only where all nchan channels are
    flagged; vis = sum(vis flagged_weight) / sum(flagged_weight) where that
    sum is positive and the output is not flagged; weight and imaging_weight
    the flagged sums; frequency the mean and channel_bandwidth the sum of the
    input's.  One kernel call (sdp_hip_vis_average_channels, variant 0)."""
    v, w, iw, fl = _operands(vis)
    out = _like(vis, *kernels.vis_average_channels(v, w, iw, fl, v.shape[2], 0))
    freq = np.asarray(vis.frequency.data)
    return _new_visibility(vis, *out,
                           np.ones([1]) * np.average(freq),
                           np.ones([1]) * np.sum(np.asarray(vis.channel_bandwidth.data)),
                           vis.visibility_acc.polarisation_frame)


def average_visibility_by_channel(vis, channel_average=None):
    """Reference visibility/operations.py:238-306: the visibility averaged
    over groups of ``channel_average`` channels, as a list of one-channel
    Visibilities (slices of one kernel call's output,
    sdp_hip_vis_average_channels, variant 1).  As in the reference the
    numerator is flagged_vis * weight and a group's flag count is compared
    with the TOTAL nchan (:292), so the output flags are 0 unless the group is
    the whole band.  Deviation: a ``channel_average`` that is None or does not
    divide nchan raises ValueError (the reference dies with a TypeError or
    IndexError)."""
    nchan = int(vis.vis.shape[2])
    if channel_average is None or int(channel_average) != channel_average \
            or channel_average < 1 or nchan % int(channel_average):
        raise ValueError(f"channel_average = {channel_average} must be an integer that divides "
                         f"nchan = {nchan}")
    G = int(channel_average)
    v, w, iw, fl = _operands(vis)
    ov, ow, oiw, ofl = _like(vis, *kernels.vis_average_channels(v, w, iw, fl, G, 1))
    freq = np.asarray(vis.frequency.data)
    cb = np.asarray(vis.channel_bandwidth.data)
    pf = vis.visibility_acc.polarisation_frame
    out = []
    for g in range(nchan // G):
        s = slice(g, g + 1)
        out.append(_new_visibility(vis, ov[:, :, s], ow[:, :, s], oiw[:, :, s], ofl[:, :, s],
                                   np.array([np.average(freq[g * G:(g + 1) * G])]),
                                   np.array([np.sum(cb[g * G:(g + 1) * G])]), pf))
    return out


def convert_visibility_to_stokes(vis):
    """Reference visibility/operations.py:309-333: linear or circular
    visibilities to stokesIQUV in place (vis <- M vis per sample with
    datamodels.pol_conversion_matrix, every pol's flag <- flag[0] | flag[3]);
    other frames are returned untouched.  One kernel pass
    (sdp_hip_vis_to_stokes)."""
    poldef = vis.visibility_acc.polarisation_frame
    if poldef.type not in ("linear", "circular"):
        return vis
    m = pol_conversion_matrix(poldef, PolarisationFrame("stokesIQUV"))
    v, _, _, fl = _operands(vis, imaging_weight=False)
    kernels.vis_to_stokes(v, fl, m)
    _write_back(vis, "vis", v)
    _write_back(vis, "flags", fl)
    vis.attrs["_polarisation_frame"] = "stokesIQUV"
    return vis


def convert_visibility_to_stokesI(vis):
    """Reference visibility/operations.py:336-420: Stokes I of linear,
    linearnp, circular or circularnp visibilities as a new Visibility (a
    stokesI input is returned as is, any other frame is a NameError).
    vis_I = 0.5 (fv[first] + fv[last]) of the FLAGGED visibilities, weight and
    imaging_weight the sums of the two hands' flagged weights, flag =
    flag[first] | flag[last]; last is pol 3 (linear, circular) or pol 1
    (linearnp, circularnp).  The reference takes vis_I from
    convert_linear_to_stokesI / convert_circular_to_stokesI of
    ska-sdp-datamodels; they are taken here to be the half-sum of the two
    parallel hands, which is what the Stokes matrices give for I."""
    poldef = vis.visibility_acc.polarisation_frame
    if poldef == PolarisationFrame("stokesI"):
        return vis
    if poldef.type not in ("linear", "linearnp", "circular", "circularnp"):
        raise NameError(f"Polarisation frame {poldef} unknown")
    v, w, iw, fl = _operands(vis)
    out = _like(vis, *kernels.vis_to_stokes_i(v, w, iw, fl))
    return _new_visibility(vis, *out, vis.frequency.data,
                           vis.channel_bandwidth.data, PolarisationFrame("stokesI"))


def convert_visibility_stokesI_to_polframe(vis, poldef=None):
    """Reference visibility/operations.py:423-471: Stokes I repeated into the
    pols of ``poldef`` as a new Visibility, pols 1 and 2 zeroed as the
    reference does (array operations, no kernel).  A 2-pol ``poldef`` raises
    ValueError: the reference indexes pol 2 out of range there."""
    if vis.visibility_acc.polarisation_frame == poldef:
        return vis
    npol = poldef.npol
    if npol < 3:
        raise ValueError(f"convert_visibility_stokesI_to_polframe: {poldef} has {npol} "
                         "polarisations, 4 are needed")
    acc = vis.visibility_acc

    def rep(a):
        a = a[..., 0:1]
        if isinstance(a, torch.Tensor):
            return a.repeat_interleave(npol, dim=-1)
        return np.repeat(np.asarray(a), npol, axis=-1)

    vis_data = rep(acc.flagged_vis)
    vis_data[..., 1] = 0.0
    vis_data[..., 2] = 0.0
    out = Visibility.constructor(
        frequency=vis.frequency.data, channel_bandwidth=vis.channel_bandwidth.data,
        phasecentre=vis.phasecentre, baselines=vis.baselines.data,
        configuration=vis.configuration, uvw=vis.uvw.data, time=vis.time.data, vis=vis_data,
        flags=rep(vis.flags.data), weight=rep(acc.flagged_weight),
        integration_time=vis.integration_time.data, polarisation_frame=poldef,
        source=vis.attrs.get("source"), meta=vis.attrs.get("meta"))
    out["imaging_weight"] = rep(acc.flagged_imaging_weight)
    return out


def _fit_deficient_on_host(v, w, fl, x, mask, degree, idx):
    """numpy.polyfit (LAPACK's minimum-norm solution, as the reference) for
    the spectra ``idx`` = row * npol + pol with fewer live channels than
    coefficients; v [t, b, f, p] is updated in place."""
    nchan, npol = v.shape[2], v.shape[3]
    rows = torch.div(idx, npol, rounding_mode="floor").long()
    pols = (idx % npol).long()
    vf = v.view(-1, nchan, npol)
    y = vf[rows, :, pols].to(torch.complex128).cpu().numpy()
    fw = (w.view(-1, nchan, npol)[rows, :, pols]
          * (1.0 - fl.view(-1, nchan, npol)[rows, :, pols].to(torch.float64))).cpu().numpy()
    for k in range(y.shape[0]):
        wt = np.sqrt(fw[k])
        if mask is not None:
            wt[mask] = 0.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fit = np.polyfit(x, y[k], w=wt, deg=degree)
        y[k] = y[k] - np.polyval(fit, x)
    vf[rows, :, pols] = torch.as_tensor(y, device=v.device).to(v.dtype)


def remove_continuum_visibility(vis, degree=1, mask=None):
    """Reference visibility/operations.py:108-142: fit a polynomial of
    ``degree`` in frequency to every (time, baseline, pol) spectrum and
    subtract it, in place.  The abscissa is x = (f - f[nchan // 2]) /
    (f[0] - f[nchan // 2]); the fit weight is flagged_weight (the reference
    hands sqrt(flagged_weight) to numpy.polyfit, which squares it); the fit is
    made to the unflagged vis and subtracted at every channel.

    ``mask``: the weight is set to 0 on the channels where mask is TRUE --
    what the reference's code does (:135-136), although its docstring says
    the fit is made where mask is True.  The assertion sum(mask) > 2 degree is
    kept.

    One kernel (sdp_hip_vis_remove_continuum) solves each spectrum in fp64
    with the orthogonal polynomials of its own weights; degrees 0 to 5 (a
    larger degree raises ValueError).  Spectra with 1 <= n_live <= degree
    live channels (non-zero fit weight) get numpy.polyfit's minimum-norm
    solution on the host, as the reference.  Deviation: a spectrum without
    any live channel is left unchanged (the reference raises LinAlgError)."""
    if mask is not None:
        mask = np.asarray(_device.like_input(mask, None) if isinstance(mask, torch.Tensor)
                          else mask, dtype=bool)
        assert np.sum(mask) > 2 * degree, "Insufficient channels for fit"
    if not 0 <= int(degree) <= kernels.MAX_CONTINUUM_DEGREE or int(degree) != degree:
        raise ValueError(f"remove_continuum_visibility: degree {degree} is not supported, the "
                         f"device fit takes degrees 0 to {kernels.MAX_CONTINUUM_DEGREE}")
    degree = int(degree)
    freq = np.asarray(vis.frequency.data, dtype=float)
    nchan = len(freq)
    if nchan < 2:
        raise ValueError("remove_continuum_visibility needs at least 2 channels")
    x = (freq - freq[nchan // 2]) / (freq[0] - freq[nchan // 2])
    v, w, _, fl = _operands(vis, imaging_weight=False)
    dev = v.device
    dmask = None if mask is None else torch.as_tensor(mask, device=dev)
    idx, count = kernels.vis_remove_continuum(v, w, fl, torch.as_tensor(x, device=dev), degree,
                                              mask=dmask)
    if count:
        if idx is None:  # more than the list holds: count the live channels here
            fw = w * (1.0 - fl.to(torch.float64))
            if dmask is not None:
                fw[:, :, dmask, :] = 0.0
            live = (fw != 0).sum(dim=2).reshape(-1)
            idx = torch.nonzero((live >= 1) & (live <= degree)).reshape(-1)
        _fit_deficient_on_host(v, w, fl, x, mask, degree, idx)
    _write_back(vis, "vis", v)
    return vis


def expand_polarizations(data, dtype=None):
    """Reference visibility/operations.py:474-503: [frequency, baselines,
    pols] data expanded to 4 pols (2 pols go to 0 and 3, 1 pol to both);
    4-pol data of the same dtype is returned as is."""
    if dtype is None:
        dtype = data.dtype
    npol = data.shape[-1]
    if npol == 4 and dtype == data.dtype:
        return data
    shape = tuple(data.shape[:-1]) + (4,)
    if isinstance(data, torch.Tensor):
        out = torch.zeros(shape, dtype=dtype, device=data.device)
    else:
        out = np.zeros(shape, dtype=dtype)
    if npol == 4:
        out[:] = data
    elif npol == 2:
        out[:, :, 0] = data[:, :, 0]
        out[:, :, 3] = data[:, :, 1]
    else:
        out[:, :, 0] = data[:, :, 0]
        out[:, :, 3] = data[:, :, 0]
    return out


def divide_visibility(vis, modelvis):
    dev = _device.device()
    v = _device.to_dev(vis["vis"].data, None, dev)
    if v.dtype not in (torch.complex64, torch.complex128):
        v = v.to(torch.complex128)
    v = v.contiguous()
    m = _device.to_dev(modelvis["vis"].data, v.dtype, dev).contiguous()
    w = _device.to_dev(vis["weight"].data, torch.float64, dev).contiguous()
    fl = _device.to_dev(vis["flags"].data, None, dev)
    if fl.dtype not in kernels.FLAG_BYTES:
        fl = fl.to(torch.int64)
    mfl = None
    if modelvis["flags"].data is not vis["flags"].data:
        mfl = _device.to_dev(modelvis["flags"].data, fl.dtype, dev)
    x, xwt = kernels.divide_vis(v, m, w, fl.contiguous(), model_flags=mfl)
    ref = vis["vis"].data
    out = Visibility.constructor(
        flags=vis.flags.data, baselines=vis.baselines.data, frequency=vis.frequency.data,
        channel_bandwidth=vis.channel_bandwidth.data, phasecentre=vis.phasecentre,
        configuration=vis.configuration, uvw=vis.uvw.data, time=vis.time.data,
        integration_time=vis.integration_time.data, vis=_device.like_input(x, ref),
        weight=_device.like_input(xwt, ref), source=vis.attrs.get("source"),
        meta=vis.attrs.get("meta"), polarisation_frame=vis.visibility_acc.polarisation_frame)
    out["imaging_weight"] = vis.imaging_weight.data
    return out
