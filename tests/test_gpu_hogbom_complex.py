"""GPU parity of the complex Hogbom clean (csrc/clean.hip's k_select_c /
k_update_c through kernels.clean_plane_complex, image.cleaners.hogbom_complex
and image.deconvolution.complex_hogbom_kernel_list) against the reference's
goldens and the numpy restatement (tests/hogbom_complex_restatement.py).

Every comparison is np.array_equal.  Exact is derivable: every golden keeps
each choice of a peak and each stop test at least 1e-9 (relative) away from a
tie, far more than hypot implementations differ by, so the device picks the
same peaks; with the same peaks every output value is the same sequence of
single IEEE fp64 operations (contraction is off in clean.hip).
"""

import functools

import numpy as np
import pytest
import torch

import clean_restatement as cr
import hogbom_complex_restatement as hr
from conftest import golden
from ska_sdp_func_python_amd import datamodels as dm
from ska_sdp_func_python_amd import kernels
from ska_sdp_func_python_amd.image import cleaners
from ska_sdp_func_python_amd.image import deconvolution as dc

pytestmark = pytest.mark.gpu


def T(a):
    return None if a is None else torch.as_tensor(np.asarray(a, dtype=float), device="cuda:0")


def H(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


@functools.lru_cache(maxsize=None)
def case(name):
    """The golden case and the restatement's cycle count, computed once."""
    c = hr.load_case(name, golden)
    c["restated_cycles"] = hr.hogbom_complex(c["dirty_q"], c["dirty_u"], c["psf"], c["window"],
                                             c["gain"], c["thresh"], c["niter"], c["fracthresh"])[4]
    for a in (c["dirty_q"], c["dirty_u"], c["psf"]) + c["expect"]:
        a.setflags(write=False)
    return c


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", hr.cases())
def test_golden(name, on_device):
    c = case(name)
    conv = T if on_device else (lambda a: a)
    args = (conv(c["dirty_q"]), conv(c["dirty_u"]), conv(c["psf"]), conv(c["psf"]),
            conv(c["window"]), c["gain"], c["thresh"], c["niter"], c["fracthresh"])
    out = cleaners.hogbom_complex_run(*args)
    assert len(out) == 5
    for got, want in zip(out[:4], c["expect"]):
        assert isinstance(got, torch.Tensor) == on_device
        print(name, "max difference", np.abs(H(got) - want).max())
        assert np.array_equal(H(got), want)
    assert out[4]["niter"] == c["restated_cycles"] == c["cycles"]
    assert out[4]["stop"] == ("threshold" if name == "C6" else "niter")
    plain = cleaners.hogbom_complex(*args)
    assert len(plain) == 4 and all(np.array_equal(H(a), H(b)) for a, b in zip(plain, out[:4]))


def test_exact_tie_takes_the_first_index_across_tiles():
    """Two peaks of equal |P| = hypot(0.6, 0.8) in different tiles, with
    different polarisation angles: bit-equal to the restatement, so the lower
    flat index wins every tie.  After an even number of cycles both have had
    the same share; at niter = 5 the first is one component ahead."""
    q, u = np.zeros((70, 70)), np.zeros((70, 70))
    q[3, 66], u[3, 66] = 0.6, 0.8
    q[40, 5], u[40, 5] = -0.6, 0.8
    psf = np.zeros((16, 16))
    psf[8, 8] = 1.0
    for niter in (6, 5):
        want = hr.hogbom_complex(q, u, psf, None, 0.5, 0.0, niter, 0.0)
        assert want[4] == niter
        assert (abs(want[0][3, 66]) > abs(want[0][40, 5])) == (niter == 5)
        assert (want[1][3, 66] > want[1][40, 5]) == (niter == 5)
        for conv in (lambda a: a, T):
            out = cleaners.hogbom_complex_run(conv(q), conv(u), conv(psf), conv(psf), None, 0.5, 0.0,
                                              niter, 0.0)
            for got, expect in zip(out[:4], want[:4]):
                assert np.array_equal(H(got), expect)
            assert out[4] == {"niter": niter, "stop": "niter"}


def test_zero_u_is_the_real_hogbom():
    """U = 0: |P| = |Q|, so the Q outputs are those of cleaners.hogbom on the
    Q plane (both thresholds 0: the two stop rules differ) and U stays exactly
    zero.  dirty_b is 67 x 45: partial tiles on both axes, an odd PSF."""
    inp = golden("clean_inputs.npz")
    q, psf = inp["dirty_b"], inp["psf_b33"]
    comps, res = cleaners.hogbom(q, psf, None, 0.1, 0.0, 40, 0.0)
    cq, cu, rq, ru, info = cleaners.hogbom_complex_run(q, np.zeros_like(q), psf, psf, None, 0.1, 0.0,
                                                       40, 0.0)
    assert np.array_equal(cq, comps) and np.array_equal(rq, res)
    assert not cu.any() and not ru.any()
    assert info == {"niter": 40, "stop": "niter"}


def test_one_cycle_through_the_kernel_entry():
    """One cycle by hand: the peak of |P| is (40, 5) although Q alone peaks at
    (3, 66); a PSF of maximum 2 halves the component."""
    q, u = np.zeros((70, 70)), np.zeros((70, 70))
    q[3, 66], u[3, 66] = 0.9, 0.0
    q[40, 5], u[40, 5] = -0.6, 0.8
    q[41, 6], u[41, 6] = 0.25, -0.5
    psf = np.zeros((16, 16))
    # row and column 15 = 2 * (16 // 2) - 1 are the last inside the patch
    psf[8, 8], psf[9, 9], psf[0, 0], psf[15, 15] = 2.0, 0.5, 0.25, 1.75
    res = T(np.stack([q, u]))
    comps = torch.zeros_like(res)
    assert kernels.clean_plane_complex(res, T(psf), comps, 0.5, 2.0, 0.0, 1) == (1, "niter")
    mq, mu = (-0.6 * 0.5) * 0.5, (0.8 * 0.5) * 0.5
    want_c = np.zeros((2, 70, 70))
    want_c[:, 40, 5] = mq, mu
    want_r = np.stack([q, u])
    for (dy, dx), t in {(0, 0): 2.0, (1, 1): 0.5, (7, 7): 1.75}.items():
        want_r[0, 40 + dy, 5 + dx] -= t * mq
        want_r[1, 40 + dy, 5 + dx] -= t * mu
    # psf[0, 0] would land on (32, -3): outside the image
    assert np.array_equal(H(comps), want_c)
    assert np.array_equal(H(res), want_r)
    assert want_r[0, 47, 12] == -1.75 * mq and want_r[1, 41, 6] == -0.5 - 0.5 * mu

    with pytest.raises(ValueError, match="res must be"):
        kernels.clean_plane_complex(res[0], T(psf), comps, 0.5, 2.0, 0.0, 1)
    with pytest.raises(ValueError, match="comps"):
        kernels.clean_plane_complex(res, T(psf), comps[0], 0.5, 2.0, 0.0, 1)
    with pytest.raises(ValueError, match="pmax"):
        kernels.clean_plane_complex(res, T(psf), comps, 0.5, 0.0, 0.0, 1)
    with pytest.raises(ValueError, match="niter"):
        kernels.clean_plane_complex(res, T(psf), comps, 0.5, 2.0, 0.0, 0)


# ---- complex_hogbom_kernel_list --------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cube():
    """The [2 chan, 4 pol] 64 x 48 dirty cube and PSF cube of
    tests/test_gpu_clean.py, rebuilt here, with one PSF for all four
    polarisations."""
    rng = np.random.default_rng(11)
    uv = rng.normal(0.0, 0.12, (200, 2))
    y, x = np.mgrid[0:64, 0:48]

    def beam(dy, dx):
        return np.cos(2 * np.pi * (uv[:, 0, None, None] * dx + uv[:, 1, None, None] * dy)).mean(0)

    psf = np.zeros((2, 4, 64, 48))
    psf[:] = beam(y - 32, x - 24)
    dirty = rng.normal(0.0, 0.02, (2, 4, 64, 48))
    for chan in range(2):
        for pol in range(4):
            for _ in range(5):
                py, px = rng.integers(8, 56), rng.integers(8, 40)
                dirty[chan, pol] += rng.uniform(0.3, 1.0) * beam(y - py, x - px)
    dirty.setflags(write=False)
    psf.setflags(write=False)
    return dirty, psf


def _image(data):
    im = dm.create_image(max(data.shape[2:]), 0.001, dm.SkyCoord(0.2, -0.7), nchan=data.shape[0])
    im["pixels"].data = data
    im.attrs["_polarisation_frame"] = "stokesIQUV"
    return im


def _lists(conv, psf=None):
    dirty, full = _cube()
    psf = full if psf is None else psf
    return ([_image(conv(dirty[c:c + 1])) for c in range(2)],
            [_image(conv(psf[c:c + 1])) for c in range(2)])


KW = dict(niter=40, gain=0.2, fractional_threshold=0.05)


@functools.lru_cache(maxsize=None)
def _planes(chan):
    """What the cleaners give for the planes of one channel (numpy input)."""
    dirty, psf = _cube()
    d, p = dirty[chan], psf[chan]
    return {0: cleaners.hogbom(d[0], p[0], None, 0.2, 0.0, 40, 0.05),
            3: cleaners.hogbom(d[3], p[3], None, 0.2, 0.0, 40, 0.05),
            "qu": cleaners.hogbom_complex(d[1], d[2], p[1], p[2], None, 0.2, 0.0, 40, 0.05)}


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
def test_list_driver_planes(on_device):
    """I and V equal cleaners.hogbom, Q and U cleaners.hogbom_complex, in both
    list entries (the reference raises IndexError on the second)."""
    dirty_list, psf_list = _lists(T if on_device else np.array)
    comps, resids = dc.complex_hogbom_kernel_list(dirty_list, psf_list, None, **KW)
    assert len(comps) == len(resids) == 2
    for chan in range(2):
        for im in (comps[chan], resids[chan]):
            assert isinstance(im["pixels"].data, torch.Tensor) == on_device
            assert im.image_acc.polarisation_frame.type == "stokesIQUV"
            assert im.image_acc.wcs is dirty_list[chan].image_acc.wcs
        c, r = H(comps[chan]["pixels"].data), H(resids[chan]["pixels"].data)
        assert c.shape == r.shape == (1, 4, 64, 48)
        want = _planes(chan)
        for pol in (0, 3):
            assert np.array_equal(c[0, pol], want[pol][0]) and np.array_equal(r[0, pol], want[pol][1])
        cq, cu, rq, ru = want["qu"]
        assert np.array_equal(c[0, 1], cq) and np.array_equal(c[0, 2], cu)
        assert np.array_equal(r[0, 1], rq) and np.array_equal(r[0, 2], ru)
        assert cq.any() and cu.any()


def test_list_driver_skips_q_and_u_on_a_zero_q_psf():
    psf = np.array(_cube()[1])
    psf[:, 1] = 0.0
    comps, resids = dc.complex_hogbom_kernel_list(*_lists(np.array, psf), None, **KW)
    for chan in range(2):
        c, r = comps[chan]["pixels"].data, resids[chan]["pixels"].data
        assert not c[0, 1:3].any() and not r[0, 1:3].any()
        assert np.array_equal(c[0, 0], _planes(chan)[0][0]) and np.array_equal(r[0, 3], _planes(chan)[3][1])


def test_list_driver_uses_the_window_of_q():
    dirty, psf = _cube()
    window = np.zeros((1, 4, 64, 48))
    window[0, 0], window[0, 3] = 1.0, 1.0
    window[0, 1, 10:40, 8:30] = 1.0
    window[0, 2, 30:60, 20:44] = 1.0
    dirty_list, psf_list = _lists(np.array)
    comps, resids = dc.complex_hogbom_kernel_list(dirty_list, psf_list, [_image(window)] * 2, **KW)
    c, r = comps[0]["pixels"].data, resids[0]["pixels"].data
    cq, cu, rq, ru = cleaners.hogbom_complex(dirty[0, 1], dirty[0, 2], psf[0, 1], psf[0, 2],
                                             window[0, 1], 0.2, 0.0, 40, 0.05)
    assert np.array_equal(c[0, 1], cq) and np.array_equal(c[0, 2], cu)
    assert np.array_equal(r[0, 1], rq) and np.array_equal(r[0, 2], ru)
    for plane in (c[0, 1], c[0, 2]):
        outside = plane.copy()
        outside[10:40, 8:30] = 0.0
        assert plane.any() and not outside.any()
    want = cr.hogbom(dirty[0, 0], psf[0, 0], window[0, 0], 0.2, 0.0, 40, 0.05)
    assert np.abs(c[0, 0] - want[0]).max() <= 1e-12
