"""Hits of the layout cache that replay the kept permutation: a kept layout's
first hit records every visibility's first-level position and the final
move's staging slots and destinations (SDP_HIP_LAYOUT_RECORD=1: the keeping
call does), the record offsets stay in place, and every later hit moves only
the 8-byte values (k_t_values, k_t_replay).  Every test therefore makes at
least two hits, and both ways of recording run.

References and bounds as tests/test_gpu_layout_cache.py: the exact direct sums
(nufft_oracle.ms2dirty_exact, wgrid_cpu.exact_pixels) at 5e-6 relative RMS,
the same call with SDP_HIP_LAYOUT_CACHE=0 at 1e-6, weight sums within 1e-12
relative.  One value behind the wrong offsets moves these images by 2e-3
(394 k visibilities) to 3e-2 (2,400), far outside both bounds.
"""

import numpy as np
import pytest
import torch

import nufft_oracle as orc
from conftest import rel_rms

pytestmark = pytest.mark.gpu
TOL = 5e-6      # against the exact sums
TOL_AB = 1e-6   # cache on against cache off
TOL_SW = 1e-12  # weight sums, relative
FLIP_UW = np.array([-1.0, 1.0, -1.0])
NPIX = 64


def dev():
    return torch.device("cuda:0")


def T(a, dt=None):
    return torch.as_tensor(np.asarray(a), device=dev(), dtype=dt)


class Problem:
    """About 300 rows x 8 channels, npix 64, epsilon 1e-7, flip_uw on."""

    def __init__(self, seed, nrow=300, nchan=8):
        rng = np.random.default_rng(seed)
        self.rng = rng
        self.freq = np.linspace(1.0e9, 1.2e9, nchan)
        umax = 2000.0
        self.uvw = rng.uniform(-1, 1, (nrow, 3)) * umax * orc.C_LIGHT / self.freq.max()
        self.uvw[:, 2] *= 0.6
        self.cell = 0.45 / umax
        self.wgt = rng.uniform(0.5, 1.5, (nrow, nchan)).astype(np.float32)
        self.uvw_t, self.freq_t = T(self.uvw), T(self.freq)
        self.shape = (nrow, nchan)

    def vis(self, dt=np.complex64):
        return (self.rng.normal(size=self.shape) +
                1j * self.rng.normal(size=self.shape)).astype(dt)

    def exact(self, ms, wgt=None, do_w=True):
        return orc.ms2dirty_exact(self.uvw * FLIP_UW, self.freq, ms,
                                  self.wgt if wgt is None else wgt, NPIX, NPIX, self.cell,
                                  self.cell, do_w)

    def run(self, ms, wgt=None, eps=1e-7, slot=0, do_w=True):
        """kernels.ms2dirty; ms / wgt host arrays or device tensors"""
        from ska_sdp_func_python_amd import kernels
        ms_t = ms if isinstance(ms, torch.Tensor) else T(ms)
        w = self.wgt if wgt is None else wgt
        w_t = w if isinstance(w, torch.Tensor) else T(w)
        out, info = kernels.ms2dirty(self.uvw_t, self.freq_t, ms_t, w_t, NPIX, NPIX, self.cell,
                                     self.cell, eps, do_w, flip_uw=True, slot=slot)
        return out.cpu().numpy(), info

    def run_vis(self, ms, wgt=None, flags=None, coef=None, **kw):
        """kernels.ms2dirty_vis (image pol 0): image, weight sum, info.  ms
        [nrow, nchan] or [nrow, nchan, npol], host array or device tensor"""
        from ska_sdp_func_python_amd import kernels
        ms_t = ms if isinstance(ms, torch.Tensor) else T(ms)
        if ms_t.dim() == 2:
            ms_t = ms_t[:, :, None]
        w = self.wgt if wgt is None else wgt
        w_t = w if isinstance(w, torch.Tensor) else T(w)
        f_t = None
        if flags is not None:
            f_t = T(flags)
            if f_t.dim() == 2:
                f_t = f_t[:, :, None].contiguous()
        sw = torch.zeros(1, dtype=torch.float64, device=dev())
        out, info = kernels.ms2dirty_vis(self.uvw_t, self.freq_t, ms_t, 0, w_t, f_t, coef, NPIX,
                                         NPIX, self.cell, self.cell, 1e-7, True, flip_uw=True,
                                         sumwt=sw, **kw)
        return out.cpu().numpy(), float(sw.cpu()), info


@pytest.fixture(params=["fold", "nofold"])
def fold(request, monkeypatch):
    monkeypatch.setenv("SDP_HIP_HFOLD", "1" if request.param == "fold" else "0")
    return request.param == "fold"


@pytest.fixture(autouse=True, params=["rec_hit", "rec_miss"])
def _record(request, monkeypatch):
    """the permutation recorded by the first hit (the default) or by the
    keeping call"""
    if request.param == "rec_miss":
        monkeypatch.setenv("SDP_HIP_LAYOUT_RECORD", "1")


@pytest.fixture(autouse=True)
def _fresh_slots():
    """no layout kept by an earlier test: the first call of every test is a miss"""
    from ska_sdp_func_python_amd import kernels
    torch.cuda.synchronize()
    kernels.release_workspace()
    yield
    torch.cuda.synchronize()


def cache_off(monkeypatch, fn):
    monkeypatch.setenv("SDP_HIP_LAYOUT_CACHE", "0")
    try:
        return fn()
    finally:
        monkeypatch.delenv("SDP_HIP_LAYOUT_CACHE")


def near(a, b):
    return abs(a - b) <= TOL_SW * abs(b)


def test_straddled_chunks_with_frozen_counts(monkeypatch):
    """The geometry of test_bins_of_several_chunks (393.6 k visibilities, two
    bins of one first plane, one of them of 3 chunks whose boundaries the
    value pass's workgroup slices straddle): five hits alternating two
    visibility sets, each against the cache-off image and 40 exact pixels."""
    import wgrid_cpu
    from ska_sdp_func_python_amd import kernels
    rng = np.random.default_rng(28)
    nrow, nchan, npix = 4100, 96, 256
    freq = np.linspace(1.00e9, 1.05e9, nchan)
    cell = 1.0e-4
    ngrid = 2 * npix
    a_u = rng.uniform(12.0, 55.0, nrow)
    a_v = rng.uniform(12.0, 55.0, nrow)
    other = rng.uniform(size=nrow) < 0.1
    lam = orc.C_LIGHT / freq.max()
    sign = np.where(rng.uniform(size=nrow) < 0.5, -1.0, 1.0)
    uvw = np.empty((nrow, 3))
    uvw[:, 0] = -sign * a_u / (cell * ngrid) * lam
    uvw[:, 1] = sign * np.where(other, -a_v, a_v) / (cell * ngrid) * lam
    uvw[:, 2] = rng.uniform(-50.0, 50.0, nrow) * lam
    wgt = rng.uniform(0.5, 1.5, (nrow, nchan)).astype(np.float32)
    uvw_t, freq_t, wgt_t = T(uvw), T(freq), T(wgt)

    def run(ms_t):
        o, i = kernels.ms2dirty(uvw_t, freq_t, ms_t, wgt_t, npix, npix, cell, cell, 1e-7, True,
                                flip_uw=True)
        return o.cpu().numpy(), i

    px = np.concatenate([[npix // 2, 0, npix - 1, npix // 2 + 1], rng.integers(0, npix, 36)])
    py = np.concatenate([[npix // 2, npix // 2, npix - 1, npix // 2 - 7], rng.integers(0, npix, 36)])
    mss = [(rng.normal(size=(nrow, nchan)) + 1j * rng.normal(size=(nrow, nchan))).astype(np.complex64)
           for _ in range(3)]
    ms_t = [T(m) for m in mss]
    _, i0 = run(ms_t[0])
    assert i0["layout_reused"] == 0 and i0["tiled"] == 1 and i0["folded"] == 1
    assert i0["nplanes"] == i0["support"] and i0["nvis_used"] == nrow * nchan
    hits = [run(ms_t[1 + k % 2]) for k in range(5)]
    assert [i["layout_reused"] for _, i in hits] == [1] * 5
    refs = []
    for k in (1, 2):
        off, io = cache_off(monkeypatch, lambda: run(ms_t[k]))
        assert io["layout_reused"] == 0
        ex = wgrid_cpu.exact_pixels(uvw * FLIP_UW, freq, mss[k], wgt, npix, npix, cell, cell, True,
                                    px, py, nthreads=4)
        assert rel_rms(off[px, py], ex) < TOL
        refs.append((off, ex))
    for k, (a, _) in enumerate(hits):
        off, ex = refs[k % 2]
        assert rel_rms(a, off) < TOL_AB, k
        assert rel_rms(a[px, py], ex) < TOL, k


@pytest.mark.parametrize("keep_dt", [np.complex64, np.complex128])
def test_value_dtype_and_layout_change_between_keep_and_hit(keep_dt, fold, monkeypatch):
    p = Problem(21)
    hit_dt = np.complex128 if keep_dt == np.complex64 else np.complex64
    ms0, ms = p.vis(keep_dt), p.vis(hit_dt)
    a, ia = p.run(ms0)
    assert ia["layout_reused"] == 0 and rel_rms(a, p.exact(ms0)) < TOL
    ex = p.exact(ms)
    off, swo, io = cache_off(monkeypatch, lambda: p.run_vis(ms))
    assert io["layout_reused"] == 0
    # (the cache-off call was a fresh plan: keep again)
    assert p.run(ms0)[1]["layout_reused"] == 0
    # the other value dtype
    b, ib = p.run(ms)
    assert ib["layout_reused"] == 1 and rel_rms(b, ex) < TOL and rel_rms(b, off) < TOL_AB
    # f64 weights
    c, ic = p.run(ms, wgt=T(p.wgt.astype(np.float64)))
    assert ic["layout_reused"] == 1 and rel_rms(c, ex) < TOL and rel_rms(c, off) < TOL_AB
    # every second channel of a wider tensor, and a transposed allocation
    wide = torch.zeros((p.shape[0], 2 * p.shape[1]), dtype=T(ms).dtype, device=dev())
    wide[:, ::2] = T(ms)
    wide[:, 1::2] = 7.0
    d, idd = p.run(wide[:, ::2])
    assert not wide[:, ::2].is_contiguous()
    assert idd["layout_reused"] == 1 and rel_rms(d, ex) < TOL and rel_rms(d, off) < TOL_AB
    tr = T(ms).t().contiguous().t()
    assert tr.stride() == (1, p.shape[0])
    e, ie = p.run(tr)
    assert ie["layout_reused"] == 1 and rel_rms(e, ex) < TOL and rel_rms(e, off) < TOL_AB
    # through ms2dirty_vis, with flags
    dead = p.rng.uniform(size=p.shape) < 0.25
    wgt0 = np.where(dead, 0.0, p.wgt).astype(np.float32)
    f, swf, i_f = p.run_vis(ms, flags=dead.astype(np.int8))
    assert i_f["layout_reused"] == 1 and rel_rms(f, p.exact(ms, wgt=wgt0)) < TOL
    offf, swof, iof = cache_off(monkeypatch, lambda: p.run_vis(ms, flags=dead.astype(np.int8)))
    assert iof["layout_reused"] == 0 and rel_rms(f, offf) < TOL_AB and near(swf, swof)
    assert near(swf, float(wgt0.astype(np.float64).sum()))


def test_phase_shift_and_pol_row_on_a_hit(fold, monkeypatch):
    p = Problem(22)
    ms0 = p.vis()
    shift = (0.003, -0.002, np.sqrt(1.0 - 0.003 ** 2 - 0.002 ** 2) - 1.0)
    ms4 = (p.rng.normal(size=p.shape + (4,)) +
           1j * p.rng.normal(size=p.shape + (4,))).astype(np.complex64)
    coef = [0.5, 0.25j, -0.25j, 0.5]
    fl4 = (p.rng.uniform(size=p.shape + (4,)) < 0.1).astype(np.int8)
    calls = [
        lambda: p.run_vis(ms0, shift_lmn=shift),
        lambda: p.run_vis(ms4, coef=coef),
        lambda: p.run_vis(ms4, coef=coef, flags=fl4, shift_lmn=shift),
    ]
    offs = [cache_off(monkeypatch, c) for c in calls]
    assert all(i["layout_reused"] == 0 for _, _, i in offs)
    # the unshifted image differs from the shifted one by far more than the bound
    a, swa, ia = p.run_vis(ms0)
    assert ia["layout_reused"] == 0 and rel_rms(a, p.exact(ms0)) < TOL
    assert rel_rms(a, offs[0][0]) > 1e-2
    for c, (off, swo, _) in zip(calls, offs):
        b, swb, ib = c()
        assert ib["layout_reused"] == 1
        assert rel_rms(b, off) < TOL_AB and near(swb, swo)


def test_single_visibility_hits(fold):
    """each hit has one non-zero visibility: its image is that visibility's
    exact sum, so its value met its own offsets in its own cell, and every
    other slot and every pad added an exact zero"""
    p = Problem(23)
    nrow, nchan = p.shape
    assert p.run(p.vis())[1]["layout_reused"] == 0
    su_u = -p.uvw[:, 0]                                   # flip_uw
    picks = [(0, 0), (nrow - 1, nchan - 1),
             (int(np.argmax(su_u < 0)), 3), (int(np.argmax(p.uvw[:, 0] > 0)), 5),
             (int(np.argmax(su_u > 0)), 1), (nrow // 2, nchan // 2), (17, 7), (nrow - 2, 0)]
    assert su_u[picks[2][0]] < 0 and p.uvw[picks[3][0], 0] > 0
    for r, c in picks:
        ms = np.zeros(p.shape, np.complex64)
        ms[r, c] = 1.5 - 0.75j
        a, ia = p.run(ms)
        assert ia["layout_reused"] == 1
        ex = orc.ms2dirty_exact(p.uvw[r:r + 1] * FLIP_UW, p.freq[c:c + 1], ms[r:r + 1, c:c + 1],
                                p.wgt[r:r + 1, c:c + 1], NPIX, NPIX, p.cell, p.cell, True)
        assert rel_rms(a, ex) < TOL, (r, c)


@pytest.mark.parametrize("shape", [(3, 2), (301, 7)])
def test_tails(shape, fold):
    p = Problem(24, *shape)
    mss = [p.vis() for _ in range(3)]
    outs = [p.run(ms) for ms in mss]
    assert [i["layout_reused"] for _, i in outs] == [0, 1, 1]
    for ms, (a, _) in zip(mss, outs):
        assert rel_rms(a, p.exact(ms)) < TOL


def test_interleaved_final_records(fold, monkeypatch):
    """SDP_HIP_RECS_SPLIT=0: the final records stay 16-byte RecC and a replay
    writes their value halves in place"""
    monkeypatch.setenv("SDP_HIP_RECS_SPLIT", "0")
    p = Problem(29, 301, 7)
    mss = [p.vis() for _ in range(4)]
    outs = [p.run(ms) for ms in mss]
    assert [i["layout_reused"] for _, i in outs] == [0, 1, 1, 1]
    for ms, (a, _) in zip(mss, outs):
        assert rel_rms(a, p.exact(ms)) < TOL
    off, _ = cache_off(monkeypatch, lambda: p.run(mss[3]))
    assert rel_rms(outs[3][0], off) < TOL_AB


def test_without_wstacking(fold, monkeypatch):
    p = Problem(25)
    ms0, ms1, ms2 = p.vis(), p.vis(), p.vis()
    a, ia = p.run(ms0, do_w=False)
    b, ib = p.run(ms1, do_w=False)      # records the permutation
    c, ic = p.run(ms2, do_w=False)      # replays it
    assert (ia["layout_reused"], ib["layout_reused"], ic["layout_reused"]) == (0, 1, 1)
    assert rel_rms(a, p.exact(ms0, do_w=False)) < TOL
    assert rel_rms(b, p.exact(ms1, do_w=False)) < TOL
    assert rel_rms(c, p.exact(ms2, do_w=False)) < TOL
    off, _ = cache_off(monkeypatch, lambda: p.run(ms2, do_w=False))
    assert rel_rms(c, off) < TOL_AB


def test_dead_visibilities_then_full_weights(fold, monkeypatch):
    p = Problem(26)
    ms = p.vis()
    dead = p.rng.uniform(size=p.shape) < 1.0 / 3.0
    wgt0 = np.where(dead, 0.0, p.wgt).astype(np.float32)
    a, swa, ia = p.run_vis(ms)
    b, swb, ib = p.run_vis(ms, wgt=wgt0)
    c, swc, ic = p.run_vis(ms)
    assert (ia["layout_reused"], ib["layout_reused"], ic["layout_reused"]) == (0, 1, 1)
    off, swo, io = cache_off(monkeypatch, lambda: p.run_vis(ms, wgt=wgt0))
    assert io["layout_reused"] == 0
    assert rel_rms(b, off) < TOL_AB and near(swb, swo)
    assert rel_rms(b, p.exact(ms, wgt=wgt0)) < TOL
    assert rel_rms(c, a) < TOL_AB and near(swc, swa)
    assert rel_rms(c, p.exact(ms)) < TOL


@pytest.mark.parametrize("between", ["predict", "fp64", "pols"])
def test_interleaved_calls_then_two_slots(between, fold):
    from ska_sdp_func_python_amd import kernels
    p = Problem(27)
    mss = [p.vis() for _ in range(4)]
    exs = [p.exact(ms) for ms in mss]
    seq = [p.run(ms) for ms in mss[:2]]
    assert [i["layout_reused"] for _, i in seq] == [0, 1]
    assert rel_rms(seq[1][0], exs[1]) < TOL
    if between == "predict":
        kernels.dirty2ms(p.uvw_t, p.freq_t, torch.ones((NPIX, NPIX), dtype=torch.float64,
                                                       device=dev()),
                         None, p.cell, p.cell, 1e-7, True, flip_uw=True)
    elif between == "fp64":
        o, i = p.run(mss[0], eps=1e-12)
        assert i["layout_reused"] == 0 and i["fp64"] == 1 and rel_rms(o, exs[0]) < TOL
    else:
        ms4 = T(np.stack([mss[k] for k in range(4)], axis=2))
        w4 = T(np.stack([p.wgt] * 4, axis=2))
        out, _ = kernels.ms2dirty_vis_pols(p.uvw_t, p.freq_t, ms4, w4, None, None, NPIX, NPIX,
                                           p.cell, p.cell, 1e-7, True, flip_uw=True)
        o = out.cpu().numpy()
        for k in range(4):
            assert rel_rms(o[k], exs[k]) < TOL, k
    a, ia = p.run(mss[2])
    b, ib = p.run(mss[3])
    assert (ia["layout_reused"], ib["layout_reused"]) == (0, 1)
    assert rel_rms(a, exs[2]) < TOL and rel_rms(b, exs[3]) < TOL
    # slots alternated on two streams, as the benchmark's pipelined step
    streams = [torch.cuda.Stream(device=dev()) for _ in range(2)]
    vis_t = [T(mss[k % 4]) for k in range(6)]
    torch.cuda.synchronize()
    outs, infos = [], []
    for k in range(6):
        with torch.cuda.stream(streams[k % 2]):
            o, i = p.run(vis_t[k], slot=k % 2)
        outs.append(o)
        infos.append(i)
    torch.cuda.synchronize()
    assert [i["layout_reused"] for i in infos] == [1, 0, 1, 1, 1, 1]
    for k in range(6):
        assert rel_rms(outs[k], exs[k % 4]) < TOL, k
