"""GPU tests of the CBF beamformer utilities: the two bandpass kernels
(sdp_hip_resample_polyfit, sdp_hip_resample_interp) and the public functions of
calibration/beamformer_utils.py against the reference's own results
(tests/golden/beamformer_*.npz, written by
tests/golden/make_golden_beamformer.py) and the tight restatement
(tests/bandpass_restatement.py).  The bounds are those of
tests/beamformer_cases.py; none comes from what the kernels give.

Largest deviations measured on an MI355X (every test prints its own as
"DEV ..."; numpy and device-tensor inputs give the same figures):

  polyfit     |device - tight|        |device - reference|     S_case
              (share of its bound)    (share of its bound)
  wide        4.7e-16 (0.090)         1.15e-13 (0.483)         1.15e-13
  narrow      3.5e-16 (0.078)         8.42e-11 (0.500)         8.42e-11
  mid         4.0e-16 (0.086)         3.09e-05 (0.500)         3.09e-05
  deg5        5.0e-16 (0.091)         2.53e-12 (0.499)         2.53e-12
  edges       5.6e-16 (0.115)         3.52e-14 (0.473)         3.49e-14
  lowband     3.4e-16 (0.063)         9.06e-15 (0.365)         9.15e-15
  kernel edges (C_in 2 ... 1000, against the tight restatement): at most 0.169
  of the rounding bound (C_in 2), 0.042-0.097 at the other sizes

  cubicspl    |device - reference| (share of (C_in + 8) eps sum |M||g|)
  wide 1.1e-15 (0.042), narrow 9.0e-16 (0.039), mid 5.6e-16 (0.018),
  lowband 1.1e-15 (0.003)

  expand_delay_phase on device tensors: 1.1e-16 (0.5 eps) with
  reference_to_centre, 2.5e-16 (1.1 eps) without; bound 4 eps
  2 x 2 and 1 x 1 products: at most 2.5e-16, 0.26 of 4 eps (|A||B|)_ij

interp equals numpy.interp bit for bit on every fixture and edge case, the
elementwise product equals numpy's bit for bit, and a row's bits are the same
alone, in a batch of 7, on a second run and in a table split by time
(all asserted).

Neither kernel takes another path at any size: every offset is formed in 64
bits, and a table past 2^31 numbers (34 GB) is not run here.
"""

import itertools

import numpy as np
import pytest
import torch

import beamformer_cases as bc
from ska_sdp_func_python_amd import kernels
from ska_sdp_func_python_amd.calibration import beamformer_utils as bu

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _table(gain, frequency):
    """A "B" table whose arrays are device tensors."""
    return bc.table(gain, frequency, convert=_dev)


# ---- the fixtures through the public functions ----------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("case", bc.RESAMPLE)
def test_resample_bandpass_fixture(case, on_device):
    g = bc.load(f"resample_{case}")
    edges, deg = bc.resample_args(g)
    gt = bc.table(g["gain"], g["frequency"], convert=_dev if on_device else None)
    label = "tensor" if on_device else "numpy"
    for alg in str(g["algs"]).split(","):
        kw = dict(edges=edges, polydeg=deg) if alg == "polyfit" else {}
        got = bu.resample_bandpass(g["frequency_out"], gt, alg=alg, **kw)
        if on_device:
            assert isinstance(got, torch.Tensor) and got.is_cuda and got.is_contiguous()
        else:
            assert isinstance(got, np.ndarray)
        assert got.dtype in (np.complex128, torch.complex128)
        assert tuple(got.shape) == g[f"out_{alg}"].shape
        if alg == "polyfit":
            bc.check_polyfit(case, _np(got), label)
        elif alg == "interp":
            assert bc.same_bits(_np(got), g["out_interp"])
        else:
            bc.check_spline(case, _np(got), label)


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensor"])
def test_expand_delay_phase_fixture(on_device):
    g = bc.load("expand")
    gt = bc.table(g["gain"], g["frequency0"], "K", convert=_dev if on_device else None)
    for tag, centre in (("centre", True), ("raw", False)):
        frequency = g["frequency"].copy()
        got = bu.expand_delay_phase(gt, frequency, reference_to_centre=centre)
        assert np.array_equal(frequency, g["frequency"]) and got.jones_type == "B"
        if on_device:
            assert all(got[v].data.is_cuda for v in ("gain", "weight", "residual"))
            d = np.max(np.abs(_np(got.gain.data) - g[f"out_{tag}"]))
            print(f"DEV tensor expand_delay_phase {tag}: {d:.2e} ({d / bc.EPS:.2f} eps)")
            assert d <= 4 * bc.EPS
        else:
            assert bc.same_bits(got.gain.data, g[f"out_{tag}"])
        assert np.all(_np(got.weight.data) == 1) and np.all(_np(got.residual.data) == 0)
        assert tuple(got.residual.data.shape) == (3, 5, 2, 2)


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("run", bc.MULTIPLY)
def test_multiply_gaintable_jones_fixture(run, on_device):
    g = bc.load("multiply")
    a, b, elem = (str(v) for v in g[f"run_{run}"])
    conv = _dev if on_device else None
    t1, t2 = bc.multiply_table(g, a, conv), bc.multiply_table(g, b, conv)
    got = bu.multiply_gaintable_jones(t1, t2, elementwise=elem == "1")
    if on_device:
        assert all(got[v].data.is_cuda for v in ("gain", "weight", "residual"))
    want = g[f"{run}_out_gain"]
    if elem == "1":
        assert bc.same_bits(_np(got.gain.data), want)
    else:
        d = np.abs(_np(got.gain.data) - want)
        bound = bc.product_bound(g[f"{a}_gain"], g[f"{b}_gain"])
        print(f"DEV {'tensor' if on_device else 'numpy'} product {run}: {d.max():.2e} "
              f"({(d / bound).max():.3f} of bound)")
        assert np.all(d <= bound)
    assert got.jones_type == str(g[f"{run}_out_jones"])
    for v in ("weight", "residual", "frequency"):
        assert bc.same_bits(_np(got[v].data), g[f"{run}_out_{v}"])


# ---- kernel edges against the tight restatement ---------------------------------
def _edge_case(rng, c_in, c_out, nrec, rows, deg, nseg):
    """Spectra, abscissae and edges: the first segment holds exactly deg + 1
    channels, the last receives no output channel (with more than one
    segment), and some output points lie below the band (NaN)."""
    nseg = min(nseg, c_in)
    deg = min(deg, c_in // nseg - 1)
    if nseg > 1:
        rest = np.linspace(deg + 1, c_in, nseg)[:-1].round().astype(int)
        edges = [0] + [int(v) for v in rest]
        assert np.all(np.diff(edges + [c_in]) >= deg + 1)
    else:
        edges = None
    f_in = 1.0e8 + 2.5e4 * np.arange(c_in) + rng.uniform(-1e3, 1e3, c_in)
    df = f_in[1] - f_in[0]
    top = f_in[edges[-1] - 1] if nseg > 1 else f_in[-1]
    # up to 0.3 channels above `top`: inside its segment's half-channel window
    # and below that of the next segment (0.8 x 27 kHz < 23 kHz between channels)
    f_out = np.sort(rng.uniform(f_in[0] - 2 * df, top + 0.3 * df, c_out))
    shape = (1, rows, c_in, nrec, nrec) if rows == 1 else (rows, 1, c_in, nrec, nrec)
    gain = rng.normal(1.0, 0.1, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))
    return f_in, f_out, gain, edges, deg, nseg


@pytest.mark.parametrize("c_in", [2, 63, 64, 65, 255, 256, 257, 1000])
def test_polyfit_kernel_edges(c_in):
    rng = np.random.default_rng(c_in)
    worst = 0.0
    for i, (nrec, deg) in enumerate(itertools.product((1, 2), (0, 3, 7))):
        nseg = (1, 2, 5)[(i + i // 3) % 3]
        rows = (1, 7)[(i + c_in) % 2]
        c_out = (1, 65, 300)[(i + c_in) % 3]
        f_in, f_out, gain, edges, deg, nseg = _edge_case(rng, c_in, c_out, nrec, rows, deg, nseg)
        got = _np(bu.resample_bandpass(f_out, _table(gain, f_in), edges=edges, polydeg=deg))
        tight, rounding, _, outside = bc.polyfit_yardstick_of(f_out, f_in, gain, edges, deg)
        assert got.shape == tight.shape
        assert np.all(np.isnan(got[:, :, outside].real) & np.isnan(got[:, :, outside].imag))
        inside = ~outside
        if nseg > 1:
            q, e, seg, ed = bu.polyfit_tables(f_out, f_in, edges, deg)
            assert ed[1] - ed[0] == deg + 1 and not np.any(seg == nseg - 1)
        if inside.any():
            ratio = (np.abs(got - tight)[:, :, inside] / rounding[:, :, inside]).max()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (c_in, c_out, nrec, rows, deg, nseg, ratio)
    print(f"DEV polyfit kernel edges C_in {c_in}: {worst:.3f} of the rounding bound")


def _split_case():
    rng = np.random.default_rng(7)
    shape = (7, 1, 300, 2, 2)
    gain = rng.normal(1.0, 0.1, shape) * np.exp(1j * rng.uniform(-3, 3, shape))
    f_in = np.linspace(1.0e8, 1.3e8, 300)
    f_out = np.linspace(0.999e8, 1.301e8, 65)
    return f_in, f_out, gain


@pytest.mark.parametrize("alg", ["polyfit", "interp"])
def test_rows_are_independent_and_runs_repeat(alg):
    f_in, f_out, gain = _split_case()
    kw = dict(edges=[0, 100, 180], polydeg=7) if alg == "polyfit" else {}
    run = lambda g: _np(bu.resample_bandpass(f_out, _table(g, f_in), alg=alg, **kw))  # noqa
    batch = run(gain)
    assert bc.same_bits(batch, run(gain))                          # a second run
    for r in (0, 3, 6):
        assert bc.same_bits(batch[r:r + 1], run(gain[r:r + 1]))    # a row alone
    assert bc.same_bits(batch, np.concatenate([run(gain[:3]), run(gain[3:])]))  # split by time


@pytest.mark.parametrize("alg", ["polyfit", "interp", "cubicspl"])
def test_non_contiguous_gain_tensor_is_accepted(alg):
    """The public function takes any strides (same bits as a contiguous copy);
    the kernel wrappers themselves refuse them."""
    f_in, f_out, gain = _split_case()
    wide = _dev(np.concatenate([gain[::-1], gain], axis=1))   # [7, 2, ...]
    view = wide[:, 1:]                                        # every other row of it
    assert not view.is_contiguous()
    gt = bc.table(gain, f_in)
    gt["gain"].data = view
    got = bu.resample_bandpass(f_out, gt, alg=alg)
    assert tuple(got.shape) == (7, 1, 65, 2, 2) and got.is_cuda
    assert bc.same_bits(_np(got), _np(bu.resample_bandpass(f_out, _table(gain, f_in),
                                                           alg=alg)))
    with pytest.raises(ValueError, match="contiguous"):
        kernels.resample_interp(view, f_in, f_out, bu.interp_intervals(f_out, f_in))


def test_kernel_wrappers_refuse_bad_tables():
    f_in, f_out, gain = _split_case()
    g = _dev(gain)
    q, e, seg, ed = bu.polyfit_tables(f_out, f_in, None, 3)
    with pytest.raises(ValueError, match="seg must lie"):
        kernels.resample_polyfit(g, q, e, np.full_like(seg, 1), ed)
    with pytest.raises(ValueError, match="ascend"):
        kernels.resample_polyfit(g, q, e, seg, np.array([0, 301], dtype=np.int32))
    with pytest.raises(ValueError, match="tables do not fit"):
        kernels.resample_polyfit(g, q[:, :-1], e, seg, ed)
    with pytest.raises(ValueError, match="degrees 0 to 7"):
        kernels.resample_polyfit(g, np.zeros((9, 300)), np.zeros((65, 9)), seg, ed)
    with pytest.raises(ValueError, match="complex128"):
        kernels.resample_polyfit(g.to(torch.complex64), q, e, seg, ed)
    with pytest.raises(ValueError, match="device"):
        kernels.resample_interp(g.cpu(), f_in, f_out, bu.interp_intervals(f_out, f_in))


@pytest.mark.parametrize("nrec", [1, 2])
def test_interp_edges_follow_numpy(nrec):
    rng = np.random.default_rng(nrec)
    c_in = 257
    f_in = np.sort(rng.uniform(1.0e8, 1.1e8, c_in))
    shape = (2, 3, c_in, nrec, nrec)
    gain = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    gain[0, 1, 100, 0, 0] = np.nan + 1j * gain[0, 1, 100, 0, 0].imag   # numpy's fallbacks
    gain[1, 2, 7] = gain[1, 2, 8] = np.inf                              # equal knots, inf - inf
    f_out = np.concatenate([
        [f_in[0] - 1e3, f_in[0] - 1.0, f_in[0], f_in[1], f_in[100], f_in[-2], f_in[-1],
         f_in[-1] + 1.0, f_in[-1] + 1e6, np.nan, 0.5 * (f_in[7] + f_in[8])],
        np.nextafter(f_in[[0, 99, 100, 256]], np.inf), np.nextafter(f_in[[1, 100, 101, 256]], -np.inf),
        rng.uniform(f_in[98], f_in[102], 40), rng.uniform(f_in[0], f_in[-1], 245)])
    assert len(f_out) == 304
    got = _np(bu.resample_bandpass(f_out, _table(gain, f_in), alg="interp"))
    for t, a, i, j in itertools.product(range(2), range(3), range(nrec), range(nrec)):
        assert bc.same_bits(got[t, a, :, i, j], np.interp(f_out, f_in, gain[t, a, :, i, j])), (t, a)
    # a single output point, and two knots only
    one = _np(bu.resample_bandpass(f_out[20:21], _table(gain, f_in), alg="interp"))
    assert bc.same_bits(one, got[:, :, 20:21])
    two = _np(bu.resample_bandpass(f_out, _table(gain[:, :, :2], f_in[:2]), alg="interp"))
    assert bc.same_bits(two[0, 0, :, 0, 0], np.interp(f_out, f_in[:2], gain[0, 0, :2, 0, 0]))
