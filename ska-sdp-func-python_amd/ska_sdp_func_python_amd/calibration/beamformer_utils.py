"""Re-channelisation of bandpass and delay solutions for CBF beamformer
calibration on MI355X (reference
``src/ska_sdp_func_python/calibration/beamformer_utils.py``).

``set_beamformer_frequencies`` (:16-89) is host arithmetic, the reference's.
``expand_delay_phase`` (:92-151) and ``multiply_gaintable_jones`` (:199-270)
work on the gain tables alone: one broadcast expression each, numpy for host
arrays and torch for device tensors, in place of the reference's loops over
channel, time and antenna.

``resample_bandpass`` (:273-329) is the hot path: the reference runs four
nested Python loops and fits every spectrum on its own.  All spectra of a
table share their abscissae and none carries weights, so each algorithm is
one linear operator along the channel axis:

``polyfit``   sdp_hip_resample_polyfit (csrc/bandpass.hip).  The host builds
              the operator factored through polynomials orthonormal on each
              segment's input channels (``polyfit_tables``, in longdouble,
              rounded once), the kernel streams the table past it.
``interp``    sdp_hip_resample_interp: numpy.interp on complex data, bit for
              bit (``interp_intervals`` does numpy's search on the host).
``cubicspl``  no kernel of its own: scipy builds the dense operator
              ``CubicSpline(freq_in, eye(C_in))(frequency_out)``, which has
              scipy's not-a-knot ends exactly, and the device applies it with
              one einsum.  Provided and correct, not the fast path; above
              ``SPLINE_OPERATOR_MAX`` input channels scipy runs on a host
              copy of the spectra.

Deviations from the reference, all in ``polyfit``:
  * an output channel that lies in no segment is NaN + NaN j, with one
    warning logged (the reference leaves numpy.empty's garbage there);
  * a segment with no more channels than ``polydeg`` raises ValueError (the
    reference returns LAPACK's minimum-norm fit with a RankWarning);
  * fewer than 2 input channels raise ValueError (the reference: IndexError);
  * degrees above ``kernels.BANDPASS_MAX_DEGREE`` raise ValueError;
  * the fit is made in the variable t = (f - mid) / half-width of the
    segment, so it is the least-squares polynomial itself even where numpy's
    fit in raw Hz loses digits or truncates a singular value.
"""

import logging

import numpy as np
import torch

from .. import _device, kernels
from ..datamodels import GainTable

log = logging.getLogger("func-python-logger")

# cubicspl: scipy's spline of eye(C_in) holds 4 (C_in - 1) C_in doubles, 0.5 GB
# at 4096 channels; beyond that the spectra go through scipy on the host
SPLINE_OPERATOR_MAX = 4096


def _is_tensor(a):
    return isinstance(a, torch.Tensor)


def _host(a):
    return a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)


def set_beamformer_frequencies(gain_table, array=None):
    """The CBF beamformer's channel centres across the table's band (:16-89).

    LOW: multiples of 781.25 kHz from the one nearest the lowest input
    channel.  MID: steps of 300 MHz / 4096 from the first input channel.
    ``array`` ("LOW" or "MID") overrides the table's configuration name.  A
    table of one channel and an unknown array return the table's frequencies
    unchanged, with a warning.

    :return: numpy array [nfreq]
    """
    array_name = gain_table.configuration.name
    frequency_gt = _host(gain_table.frequency.data)
    nfrequency_gt = len(frequency_gt)

    if nfrequency_gt <= 1:
        log.warning("Cannot rechannelise %d channel[s]", nfrequency_gt)
        return frequency_gt

    if array is None:
        if array_name.find("LOW") == 0:
            array = "LOW"
        elif array_name.find("MID") == 0:
            array = "MID"

    if array == "LOW":
        log.debug("Setting SKA-Low CBF beamformer frequencies")
        dfrequency_bf = 781.25e3
        starting_freq_bf = dfrequency_bf * np.round(np.amin(frequency_gt) / dfrequency_bf)
    elif array == "MID":
        log.debug("Setting SKA-Mid CBF beamformer frequencies")
        dfrequency_bf = 300.0e6 / 4096
        starting_freq_bf = np.amin(frequency_gt)
    else:
        log.warning("Unknown array: %s. Frequencies unchanged", array_name)
        return frequency_gt

    frequency_bf = np.arange(starting_freq_bf, np.amax(frequency_gt), dfrequency_bf)

    log.info("Setting bandpass calibration frequencies for %s CBF", array)
    log.info(" - %d input frequency channels", nfrequency_gt)
    log.info(" - input channel width: %.2f kHz, starting at %.2f MHz",
             (frequency_gt[1] - frequency_gt[0]) / 1e3, frequency_gt[0] / 1e6)
    log.info(" - %d output frequency channels", len(frequency_bf))
    log.info(" - output channel width: %.2f kHz, starting at %.2f MHz",
             dfrequency_bf / 1e3, frequency_bf[0] / 1e6)
    return frequency_bf


def expand_delay_phase(gain_table, frequency, reference_to_centre=True):
    """A "K" table's phases at its single reference frequency expanded to
    ``frequency`` with phase = 2 pi t_delay frequency (:92-151): a "B" table
    with unit weight and zero residual.  With ``reference_to_centre`` the
    phase at the reference frequency is zero.  ``frequency`` is only read
    (the reference's ``freq -= frequency0`` changes its loop variable alone).
    """
    if gain_table.jones_type != "K":
        raise ValueError(f"Wrong Jones type: {gain_table.jones_type} != K")
    if gain_table.frequency.shape[0] != 1:
        raise ValueError("Expect a single frequency")
    frequency0 = _host(gain_table.frequency.data)[0]

    freq = np.array(_host(frequency), dtype=float)  # a copy
    if reference_to_centre:
        freq = freq - frequency0
    g = gain_table.gain.data
    shape = list(g.shape)
    shape[2] = len(freq)
    if _is_tensor(g):
        # the reference's 1j * freq / frequency0 * phase0 has the real part
        # +-0 and the imaginary part (freq / frequency0) * phase0
        phase0 = torch.angle(g.to(torch.complex128))
        ratio = torch.as_tensor(freq / frequency0, device=g.device)
        theta = ratio[None, None, :, None, None] * phase0[:, :, 0:1]
        gain = torch.polar(torch.ones_like(theta), theta)
        weight = torch.ones(shape, dtype=torch.float64, device=g.device)
        residual = torch.zeros((shape[0], shape[2], shape[3], shape[4]), dtype=torch.float64,
                               device=g.device)
    else:
        phase0 = np.angle(np.asarray(g))
        gain = np.exp((1j * freq / frequency0)[None, None, :, None, None] * phase0[:, :, 0:1])
        weight = np.ones(shape)
        residual = np.zeros((shape[0], shape[2], shape[3], shape[4]))

    return GainTable.constructor(
        gain=gain, time=gain_table.time.data, interval=gain_table.interval.data, weight=weight,
        residual=residual, frequency=_host(frequency), receptor_frame=gain_table.receptor_frame1,
        phasecentre=gain_table.phasecentre, configuration=gain_table.configuration,
        jones_type="B")


def _set_gaintable_product_shape(gain_table1, gain_table2, elementwise=False):
    """The shape of the product of two GainTables, after the reference's checks (:154-196)."""
    shape1 = tuple(gain_table1.gain.shape)
    shape2 = tuple(gain_table2.gain.shape)
    if shape1[0] != shape2[0]:
        raise ValueError(f"time error {shape1[0]} != {shape2[0]}")
    if shape1[1] != shape2[1]:
        raise ValueError(f"antenna error {shape1[1]} != {shape2[1]}")
    # the same number of channels, unless one table is constant over the band
    if shape1[2] != shape2[2] and shape1[2] != 1 and shape2[2] != 1:
        raise ValueError(f"frequency error {shape1} != {shape2}")
    if elementwise:
        if shape1[3] != shape2[3]:
            raise ValueError(f"pol error {shape1[3]} != {shape2[3]}")
        if shape1[4] != shape2[4]:
            raise ValueError(f"pol error {shape1[4]} != {shape2[4]}")
    elif gain_table1.receptor2.shape != gain_table2.receptor1.shape:
        raise ValueError("Matrices not compatible for multiplication")
    return shape1[0], shape1[1], max(shape1[2], shape2[2]), shape1[3], shape2[4]


def multiply_gaintable_jones(gain_table1, gain_table2, elementwise=False):
    """gain_table1 Jones * gain_table2 Jones for all times, antennas and
    channels, as a new table (:199-270).  A table of one channel is broadcast
    over the other's channels.  ``elementwise`` multiplies element by element
    instead (factors of one effect that combine outside the Jones formalism).
    Frequency, weight and residual are table 1's unless it has one channel;
    the jones_type is the tables' own if they agree, else "B"."""
    if gain_table1.jones_type == "K" or gain_table2.jones_type == "K":
        raise ValueError("Cannot multiply delays. Use expand_delay_phase")
    _set_gaintable_product_shape(gain_table1, gain_table2, elementwise)

    a, b = gain_table1.gain.data, gain_table2.gain.data
    if _is_tensor(a) or _is_tensor(b):
        dev = b.device if _is_tensor(b) else a.device
        a = _device.to_dev(a, torch.complex128, dev)
        b = _device.to_dev(b, torch.complex128, dev)
    else:
        a = np.asarray(a, dtype="complex128")
        b = np.asarray(b, dtype="complex128")
    if elementwise and _is_tensor(a):
        # numpy's complex product is fma(ar, b, rnd(ai * swap(b))) where the CPU
        # has fused multiply-add.  The device compiler contracts x * y to
        # fma(xi, yr, rnd(xr * yi)) in the imaginary part, so b * a has
        # numpy's bits and a * b has not (the real parts agree either way);
        # tests/test_gpu_beamformer.py pins it.
        gain = b * a
    elif elementwise:
        gain = a * b
    else:
        # sum_k a[..., i, k] * b[..., k, j], the terms added in ascending k
        gain = (a[..., :, :, None] * b[..., None, :, :]).sum(-2)

    first = gain_table1 if gain_table1.gain.shape[2] > 1 else gain_table2
    if gain_table1.jones_type == gain_table2.jones_type:
        jones_type = gain_table1.jones_type
    else:
        jones_type = "B"
    return GainTable.constructor(
        gain=gain, time=gain_table1.time.data, interval=gain_table1.interval.data,
        weight=first.weight.data, residual=first.residual.data,
        frequency=_host(first.frequency.data), receptor_frame=gain_table1.receptor_frame1,
        phasecentre=gain_table1.phasecentre, configuration=gain_table1.configuration,
        jones_type=jones_type)


# ---------------------------------------------------------------------------
# host tables of the resamplers
# ---------------------------------------------------------------------------
def normalise_edges(edges, nfrequency):
    """``PolynomialInterpolator.set_edges``' normalisation (:361-379): None or
    an empty list is the full band, and channel 0 and ``nfrequency`` are put
    in front and behind where they are missing."""
    if edges is None or len(edges) == 0:
        edges = np.array([0, nfrequency])
        log.debug("set edges to %s", edges)
    if edges[0] > 0:
        edges = np.concatenate(([0], edges))
    if edges[-1] < nfrequency:
        edges = np.concatenate((edges, [nfrequency]))
    return edges


def polyfit_tables(freq_out, freq_in, edges, polydeg):
    """(q [polydeg + 1, C_in], e [C_out, polydeg + 1], seg [C_out] int32,
    edges [nseg + 1] int32): the least-squares fit of degree ``polydeg`` per
    segment of ``edges`` (normalised) as sdp_hip_resample_polyfit takes it.

    Per segment the abscissa is t = (f - mid) / half-width of its input
    channels and p_0 .. p_polydeg are orthonormal under the unit-weight inner
    product on them, built by the three-term recurrence in longdouble and
    rounded once.  ``seg`` follows the reference's sequential assignment
    (:411-417): the half-channel window on freq_in[1] - freq_in[0], the last
    matching segment wins, -1 where none matches."""
    freq_in = np.asarray(freq_in, dtype=float)
    freq_out = np.asarray(freq_out, dtype=float)
    c_in, c_out = len(freq_in), len(freq_out)
    if c_in < 2:
        raise ValueError(f"Cannot fit {c_in} channel[s]: at least 2 are needed")
    if int(polydeg) != polydeg or not 0 <= polydeg <= kernels.BANDPASS_MAX_DEGREE:
        raise ValueError(f"polydeg {polydeg}: the fit takes integer degrees 0 to "
                         f"{kernels.BANDPASS_MAX_DEGREE}")
    polydeg = int(polydeg)
    edges = np.asarray(normalise_edges(edges, c_in))
    if not np.all(edges == np.round(edges)):
        raise ValueError(f"edges {edges} must be channel indices")
    edges = edges.astype(np.int64)
    if edges[0] < 0 or edges[-1] > c_in or np.any(np.diff(edges) < 0):
        raise ValueError(f"edges {edges} must ascend within 0 .. {c_in}")
    nseg, nd = len(edges) - 1, polydeg + 1
    if nseg > kernels.BANDPASS_MAX_SEGMENTS:
        raise ValueError(f"{nseg} segments: the fit takes at most {kernels.BANDPASS_MAX_SEGMENTS}")
    for k in range(nseg):
        if edges[k + 1] - edges[k] <= polydeg:
            raise ValueError(f"segment {k} (channels {edges[k]} .. {edges[k + 1] - 1}) has no "
                             f"more channels than polydeg = {polydeg}")
    seg = np.full(c_out, -1, dtype=np.int32)
    dfreq_in = freq_in[1] - freq_in[0]
    for k in range(nseg):
        seg[(freq_out >= freq_in[edges[k]] - dfreq_in / 2)
            & (freq_out < freq_in[edges[k + 1] - 1] + dfreq_in / 2)] = k

    ld = np.longdouble
    q = np.zeros((nd, c_in), dtype=ld)
    e = np.zeros((c_out, nd), dtype=ld)
    for k in range(nseg):
        lo, hi = edges[k], edges[k + 1]
        sel = seg == k
        f = freq_in[lo:hi].astype(ld)
        mid = (f.max() + f.min()) / 2
        half = (f.max() - f.min()) / 2
        if not half > 0:
            half = ld(1)
        t, t_out = (f - mid) / half, (freq_out[sel].astype(ld) - mid) / half
        p0 = 1 / np.sqrt(ld(hi - lo))
        p, p_out = np.full(t.shape, p0), np.full(t_out.shape, p0)
        p_prev, p_out_prev, beta = np.zeros_like(p), np.zeros_like(p_out), ld(0)
        for d in range(nd):
            q[d, lo:hi] = p
            e[sel, d] = p_out
            if d == polydeg:
                break
            alpha = np.sum(t * p * p)
            r, r_out = (t - alpha) * p - beta * p_prev, (t_out - alpha) * p_out - beta * p_out_prev
            norm = np.sqrt(np.sum(r * r))
            if not norm > 0:
                raise ValueError(f"segment {k} has fewer than {nd} distinct frequencies")
            p_prev, p_out_prev, beta = p, p_out, norm
            p, p_out = r / norm, r_out / norm
    return q.astype(np.float64), e.astype(np.float64), seg, edges.astype(np.int32)


def interp_intervals(freq_out, freq_in):
    """The knot interval of every output point as numpy.interp finds it, in
    sdp_hip_resample_interp's encoding: -2 a NaN point, -1 below the first
    knot, j for freq_in[j] <= f < freq_in[j + 1], C_in - 1 at or above the
    last knot.  ``freq_in`` ascends."""
    freq_in = np.asarray(freq_in, dtype=float)
    freq_out = np.asarray(freq_out, dtype=float)
    j = np.searchsorted(freq_in, freq_out, side="right") - 1
    j[freq_out < freq_in[0]] = -1
    j[freq_out > freq_in[-1]] = len(freq_in) - 1
    j[np.isnan(freq_out)] = -2
    return j.astype(np.int32)


def spline_operator(freq_out, freq_in):
    """[C_out, C_in]: scipy's CubicSpline (not-a-knot ends) as the linear map
    it is in the data, the system depending on ``freq_in`` alone."""
    from scipy.interpolate import CubicSpline
    freq_in = np.asarray(freq_in, dtype=float)
    return CubicSpline(freq_in, np.eye(len(freq_in)))(np.asarray(freq_out, dtype=float))


# ---------------------------------------------------------------------------
class PolynomialInterpolator:
    """Polynomial fits per sub-band of one spectrum on the host (:332-432),
    through the tables the device path uses.

    ``edges``: the starting channels of the sub-bands that are fitted
    separately (default: the full band; kept as [0, ..., nchan]).
    ``polydeg``: the degree of the fit (default 3)."""

    def __init__(self):
        self.edges = None
        self.polydeg = 3

    def set_edges(self, edges, nfrequency):
        """The start channels of the sub-bands requiring separate fits."""
        self.edges = normalise_edges(edges, nfrequency)

    def set_polydeg(self, polydeg):
        """The degree of the fitting polynomial."""
        self.polydeg = polydeg

    def tables(self, freq_out, freq_in):
        edges = self.edges
        if edges is None or len(edges) < 2:
            self.set_edges(edges, len(freq_in))
            edges = self.edges
        return polyfit_tables(freq_out, freq_in, edges, self.polydeg)

    def interp(self, freq_out, freq_in, gain):
        """The complex sequence ``gain`` [len(freq_in)] at ``freq_out``."""
        q, e, seg, edges = self.tables(freq_out, freq_in)
        gain = np.asarray(gain, dtype="complex128")
        gain_out = np.full(len(seg), np.nan + 1j * np.nan, dtype="complex128")
        for k in range(len(edges) - 1):
            sel = seg == k
            coef = q[:, edges[k]:edges[k + 1]] @ gain[edges[k]:edges[k + 1]]
            gain_out[sel] = e[sel] @ coef
        return gain_out


class NumpyLinearInterpolator:  # pylint: disable=too-few-public-methods
    """numpy.interp of one spectrum on the host (:438-461)."""

    def interp(self, freq_out, freq_in, gain):
        """The complex sequence ``gain`` [len(freq_in)] at ``freq_out``."""
        return np.interp(freq_out, freq_in, gain)


class ScipySplineInterpolator:  # pylint: disable=too-few-public-methods
    """scipy's CubicSpline through one spectrum on the host (:467-491)."""

    def interp(self, freq_out, freq_in, gain):
        """The complex sequence ``gain`` [len(freq_in)] at ``freq_out``."""
        from scipy.interpolate import CubicSpline
        return CubicSpline(freq_in, gain)(freq_out)


def resample_bandpass(frequency_out, gain_table, alg="polyfit", edges=None, polydeg=None):
    """Every spectrum of gain or leakage terms of ``gain_table`` at
    ``frequency_out`` (:273-329): [time, ant, len(frequency_out), rec, rec]
    complex128, a numpy array for a numpy table and a device tensor for a
    device-tensor table.

    ``alg``: "polyfit" (default; a polynomial of degree ``polydeg``, default
    3, through the real and the imaginary part of each sub-band of ``edges``),
    "interp" (numpy.interp) or "cubicspl" (scipy's CubicSpline)."""
    frequency_gt = np.asarray(_host(gain_table.frequency.data), dtype=float)
    frequency_out = np.asarray(_host(frequency_out), dtype=float)

    if alg == "polyfit":
        interpolator = PolynomialInterpolator()
        if edges is not None:
            interpolator.set_edges(edges, len(frequency_gt))
        if polydeg is not None:
            interpolator.set_polydeg(polydeg)
    elif alg not in ("interp", "cubicspl"):
        raise ValueError(f"unknown resampler {alg}")

    gain = gain_table.gain.data
    if alg == "polyfit":
        tables = interpolator.tables(frequency_out, frequency_gt)
    dev = gain.device if _device.is_device(gain) else _device.device()
    g = _device.to_dev(gain, torch.complex128, dev).contiguous()
    shape_out = list(g.shape)
    shape_out[2] = len(frequency_out)
    if len(frequency_out) == 0 or g.numel() == 0:
        return _device.like_input(torch.empty(shape_out, dtype=torch.complex128, device=dev), gain)

    if alg == "polyfit":
        if np.any(tables[2] < 0):
            log.warning("resample_bandpass: %d output channel[s] lie in no segment of the input "
                        "band and are set to NaN", int(np.sum(tables[2] < 0)))
        out = kernels.resample_polyfit(g, *tables)
    elif alg == "interp":
        out = kernels.resample_interp(g, frequency_gt, frequency_out,
                                      interp_intervals(frequency_out, frequency_gt))
    elif len(frequency_gt) > SPLINE_OPERATOR_MAX:
        log.info("resample_bandpass: cubicspl on %d input channels runs scipy on a host copy "
                 "of the spectra", len(frequency_gt))
        from scipy.interpolate import CubicSpline
        host = CubicSpline(frequency_gt, g.cpu().numpy(), axis=2)(frequency_out)
        out = torch.as_tensor(np.ascontiguousarray(host, dtype="complex128"), device=dev)
    else:
        op = torch.as_tensor(spline_operator(frequency_out, frequency_gt), device=dev)
        out = torch.view_as_complex(
            torch.einsum("oc,tacijk->taoijk", op, torch.view_as_real(g)).contiguous())
    return _device.like_input(out, gain)
