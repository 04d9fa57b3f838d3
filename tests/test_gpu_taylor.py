"""GPU tests of the plane-mixing kernel (csrc/taylor.hip through
kernels.mix_planes) and of the Taylor-term functions of image/taylor_terms.py
on device tensors.

Every comparison is bitwise, the signs of zeros included: the kernel starts
each output element from +0.0 and adds float64 products in ascending input
order, one rounding per product and per sum, which is what numpy's
``out[k] += in[c] * w`` does (taylor_case.mix_loop, and the numpy path of the
image functions, which tests/test_taylor_cpu.py holds against the reference).
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from ska_sdp_func_python_amd import _lib, kernels
from ska_sdp_func_python_amd.image import taylor_terms as tt

import taylor_case as T

pytestmark = pytest.mark.gpu

R = kernels.MIX_PLANES_REGS
NPIX = [1, 2, 3, 221, 4096, 4097, 70001]
# nout <= R: one pass that streams the inputs; nin <= R < nout: one pass that
# streams the outputs; both above R: passes of R outputs
COUNTS = [(1, 1), (7, 3), (3, 7), (R + 5, R + 2), (R + 2, R + 5), (3, 2 * R), (R, R + 1),
          (1, R + 3)]
DTYPES = [np.float64, np.float32]


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())  # a copy: the cached cases are read-only


def same_bits(got, want):
    """float64 device tensor against a float64 numpy array, bit for bit."""
    want = _t(np.asarray(want, dtype=np.float64))
    return got.dtype == torch.float64 and got.shape == want.shape and \
        torch.equal(got.contiguous().view(torch.int64), want.view(torch.int64))


@functools.lru_cache(maxsize=None)
def case(npix, nin, nout, dtype):
    """Inputs with -0.0 in every fourth pixel, weights with 0, 1 and -1 among
    normal deviates of either sign, and the numpy loop's result."""
    rng = np.random.default_rng(1000 * nin + nout + npix)
    x = rng.normal(size=(nin, npix)).astype(dtype)
    x[:, ::4] = -0.0
    w = rng.normal(size=(nout, nin))
    w.flat[::3] = 0.0
    w.flat[1::5] = 1.0
    w.flat[2::7] = -1.0
    want = T.mix_loop(w, list(x))
    for a in (x, w, want):
        a.setflags(write=False)
    return x, w, want


def planes(host, layout, fill=None):
    """Device planes of host [n, npix]: slices of one cube -- with an odd npix
    the odd planes are aligned to 8 bytes only, float32 ones to 4 -- or, for
    "mixed", every other plane, the first included, a tensor of its own."""
    cube = _t(host) if fill is None else torch.full(host.shape, fill, dtype=torch.float64,
                                                    device=_dev())
    out = [cube[k] for k in range(cube.shape[0])]
    if layout == "mixed":
        out = [p if k % 2 else p.clone() for k, p in enumerate(out)]
    return out


@pytest.mark.parametrize("layout", ["cube", "mixed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nin,nout", COUNTS)
@pytest.mark.parametrize("npix", NPIX)
def test_mix_planes_matches_numpy_bit_for_bit(npix, nin, nout, dtype, layout):
    x, w, want = case(npix, nin, nout, dtype)
    ins = planes(x, layout)
    outs = planes(np.empty((nout, npix)), layout, fill=np.nan)
    if npix % 2:
        assert any(p.data_ptr() % 16 for p in ins) or nin == 1
    got = kernels.mix_planes(ins, w, outs)
    assert got is outs
    assert same_bits(torch.stack(outs), want)
    assert same_bits(torch.stack(ins).double(), x.astype(np.float64))


def test_mix_planes_takes_a_cube_and_allocates_the_outputs():
    x, w, want = case(2 * 17 * 13, 5, 3, np.float64)
    cube = _t(x).reshape(5, 2, 17, 13)
    got = kernels.mix_planes(cube, w)
    assert got.shape == (3, 2, 17, 13) and got.is_cuda
    assert same_bits(got.reshape(3, -1), want)
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    again = torch.full_like(got, np.nan)
    kernels.mix_planes(cube, w, again, stream=side)
    side.synchronize()
    assert same_bits(again.reshape(3, -1), want)


def test_mix_planes_past_two_to_the_31_pixels():
    """One float32 plane of 2^31 + 3 pixels: pixel indices and byte offsets
    beyond 32 bits (8.6 GB in, 17.2 GB out)."""
    npix = 2 ** 31 + 3
    x = torch.empty(npix, dtype=torch.float32, device=_dev())
    x.copy_(torch.arange(npix, device=_dev(), dtype=torch.int64).remainder_(1021).sub_(510))
    got = kernels.mix_planes([x], [[-1.5], [0.25]])
    for k, wk in enumerate((-1.5, 0.25)):
        want = (x.double() * wk).add_(0.0)
        assert torch.equal(got[k].view(torch.int64), want.view(torch.int64))
        del want
    tail = np.arange(npix - 5, npix) % 1021 - 510.0
    assert np.array_equal(got[0, -5:].cpu().numpy(), 0.0 + -1.5 * tail)


# ---- the NaN flag ---------------------------------------------------------------------
@pytest.mark.parametrize("nin,nout", [(3, 2), (2, R + 1), (R + 2, R + 5)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_mix_planes_nan_flag(nin, nout, dtype):
    x, w, want = case(4097, nin, nout, dtype)
    w = np.where(w == 0.0, 0.5, w)
    out, flags = kernels.mix_planes(planes(x, "cube"), w, check_nan=True)
    assert flags == 0
    bad = x.copy()
    bad[-1, -1] = np.nan
    out, flags = kernels.mix_planes(planes(bad, "cube"), w, check_nan=True)
    assert flags == kernels.MIX_NAN_INPUT | kernels.MIX_NAN_OUTPUT
    assert torch.isnan(out[:, -1]).all() and not torch.isnan(out[:, :-1]).any()
    # inf * 0: a NaN output without any NaN input
    inf = x.copy()
    inf[0, 100] = np.inf
    w0 = w.copy()
    w0[-1, 0] = 0.0
    with np.errstate(invalid="ignore"):
        want = T.mix_loop(w0, list(inf))
    out, flags = kernels.mix_planes(planes(inf, "cube"), w0, check_nan=True)
    assert flags == kernels.MIX_NAN_OUTPUT
    assert np.isnan(want[-1, 100]) and np.isnan(want).sum() == 1 and same_bits(out, want)
    # without the check the call returns the outputs alone
    assert isinstance(kernels.mix_planes(planes(inf, "cube"), w0), torch.Tensor)


# ---- arguments ------------------------------------------------------------------------
def test_mix_planes_refuses_bad_arguments():
    x, w, _ = case(221, 3, 7, np.float64)
    cube = _t(x)
    ins = [cube[k] for k in range(3)]
    with pytest.raises(ValueError, match="overlaps an input"):
        kernels.mix_planes(ins, w[:1], [cube[1]])
    both = torch.zeros(442, dtype=torch.float64, device=_dev())
    with pytest.raises(ValueError, match="overlaps an input"):
        kernels.mix_planes([both[:221]], w[:1, :1], [both[110:331]])
    with pytest.raises(ValueError, match="output planes overlap"):
        kernels.mix_planes(ins, w[:2], [both[:221], both[110:331]])
    wide = torch.zeros((3, 442), dtype=torch.float64, device=_dev())
    with pytest.raises(ValueError, match="contiguous"):
        kernels.mix_planes([wide[k, ::2] for k in range(3)], w)
    with pytest.raises(ValueError, match="contiguous"):
        kernels.mix_planes(ins, w[:3], [wide[k, ::2] for k in range(3)])
    with pytest.raises(ValueError, match="weights must be"):
        kernels.mix_planes(ins, w[:, :2])
    with pytest.raises(ValueError, match="agree in dtype"):
        kernels.mix_planes(ins[:2] + [ins[2].float()], w)
    with pytest.raises(ValueError, match="float64"):
        kernels.mix_planes(ins, w[:1], [torch.zeros(221, dtype=torch.float32, device=_dev())])
    with pytest.raises(ValueError, match="device"):
        kernels.mix_planes([p.cpu() for p in ins], w)
    many = kernels.MIX_PLANES_MAX + 1
    with pytest.raises(ValueError, match="at most"):
        kernels.mix_planes([ins[0]] * many, np.zeros((1, many)))
    # the library's own checks
    out = torch.zeros(221, dtype=torch.float64, device=_dev())
    tab = (ctypes.c_void_p * many)(*([ins[0].data_ptr()] * many))
    otab = (ctypes.c_void_p * 1)(out.data_ptr())
    wts = np.zeros(many)

    def call(nin, nout, npix, in_tab, dtype=_lib.SDP_HIP_F64):
        _lib.call("sdp_hip_mix_planes", nin, nout, npix, ctypes.cast(in_tab, ctypes.c_void_p),
                  dtype, ctypes.cast(otab, ctypes.c_void_p), ctypes.c_void_p(wts.ctypes.data),
                  ctypes.POINTER(ctypes.c_int)(), kernels.stream(_dev()))

    with pytest.raises(ValueError, match="at most 4096"):
        call(many, 1, 221, tab)
    with pytest.raises(ValueError, match="at least one"):
        call(0, 1, 221, tab)
    with pytest.raises(ValueError, match="plane size"):
        call(1, 1, 0, tab)
    with pytest.raises(ValueError, match="float32 or float64"):
        call(1, 1, 221, tab, _lib.SDP_HIP_C64)
    with pytest.raises(ValueError, match="null"):
        call(2, 1, 221, (ctypes.c_void_p * 2)(ins[0].data_ptr(), None))
    call(1, 1, 221, tab)
    torch.cuda.synchronize()
    assert same_bits(out, np.zeros(221))


# ---- the image functions on device tensors -----------------------------------------------
@pytest.fixture(scope="module")
def g():
    return golden("taylor_cube.npz")


def pixels_of(g, tag):
    return g["cube"].astype(np.float32) if tag else g["cube"]


@pytest.mark.parametrize("tag", ["", "_f32"])
def test_cube_functions_on_the_device_equal_the_cpu_path(g, tag):
    host = pixels_of(g, tag)
    rf = float(g["explicit_reference"])
    for ref in (None, rf):
        im_h, im_d = T.make_cube(host), T.make_cube(_t(host))
        mom_h = tt.calculate_image_frequency_moments(im_h, reference_frequency=ref, nmoment=3)
        mom_d = tt.calculate_image_frequency_moments(im_d, reference_frequency=ref, nmoment=3)
        assert mom_d["pixels"].data.is_cuda and same_bits(mom_d["pixels"].data, mom_h["pixels"].data)
        assert same_bits(mom_d["pixels"].data, g["moments3" + ("_ref" if ref else "") + tag])
        assert mom_d.image_acc.wcs.wcs.ctype[3] == "MOMENT"
        assert im_d.image_acc.wcs.wcs.ctype[3] == "FREQ"
        back_d = tt.calculate_image_from_frequency_taylor_terms(im_d, mom_d, reference_frequency=ref)
        back_h = tt.calculate_image_from_frequency_taylor_terms(T.make_cube(g["cube"]), mom_h,
                                                                reference_frequency=ref)
        assert back_d["pixels"].data.is_cuda and same_bits(back_d["pixels"].data, back_h["pixels"].data)
        assert back_d.image_acc.wcs is im_d.image_acc.wcs
        # float32 Taylor terms are promoted before the multiply
        t32_d = T.make_cube(mom_d["pixels"].data.float())
        t32_h = T.make_cube(mom_h["pixels"].data.astype(np.float32))
        assert same_bits(
            tt.calculate_image_from_frequency_taylor_terms(im_d, t32_d)["pixels"].data,
            tt.calculate_image_from_frequency_taylor_terms(T.make_cube(g["cube"]), t32_h)["pixels"].data)


@pytest.mark.parametrize("tag", ["", "_f32"])
@pytest.mark.parametrize("nmoment", [1, 3])
def test_decoupled_terms_on_the_device_equal_the_cpu_path(g, tag, nmoment):
    host = pixels_of(g, tag)
    terms_h = tt.calculate_frequency_taylor_terms_from_image_list(T.make_list(host), nmoment=nmoment)
    terms_d = tt.calculate_frequency_taylor_terms_from_image_list(T.make_list(_t(host)),
                                                                  nmoment=nmoment)
    assert len(terms_d) == nmoment
    for d, h in zip(terms_d, terms_h):
        assert d["pixels"].data.is_cuda and same_bits(d["pixels"].data, h["pixels"].data)
        w = d.image_acc.wcs.wcs
        assert (w.ctype[3], w.crval[3], w.cunit[3]) == ("FREQ", g["frequency"][2], "Hz")


def test_list_functions_on_the_device_equal_the_cpu_path(g):
    list_h, list_d = T.make_list(g["cube"]), T.make_list(_t(g["cube"]))
    for ref in (None, float(g["explicit_reference"])):
        mom_h = tt.calculate_image_list_frequency_moments(list_h, reference_frequency=ref, nmoment=3)
        mom_d = tt.calculate_image_list_frequency_moments(list_d, reference_frequency=ref, nmoment=3)
        assert mom_d["pixels"].data.is_cuda and same_bits(mom_d["pixels"].data, mom_h["pixels"].data)
        assert same_bits(mom_d["pixels"].data, g["moments3_ref" if ref else "moments3"])
        back_h = tt.calculate_image_list_from_frequency_taylor_terms(list_h, mom_h,
                                                                     reference_frequency=ref)
        back_d = tt.calculate_image_list_from_frequency_taylor_terms(list_d, mom_d,
                                                                     reference_frequency=ref)
        assert len(back_d) == T.NCHAN
        for chan, (d, h) in enumerate(zip(back_d, back_h)):
            assert d["pixels"].data.is_cuda and d["pixels"].data.shape == (1, T.NPOL, T.NY, T.NX)
            assert same_bits(d["pixels"].data, h["pixels"].data)
            assert same_bits(d["pixels"].data[0], g["rebuilt_ref" if ref else "rebuilt"][chan])


def test_cube_moments_report_nans_from_the_device(g):
    pixels = g["cube"].copy()
    pixels[-1, -1, -1, -1] = np.nan
    with pytest.raises(AssertionError, match="NaNs present in image data"):
        tt.calculate_image_frequency_moments(T.make_cube(_t(pixels)), nmoment=2)
    pixels = g["cube"].copy()
    pixels[2, 0, 4, 4] = np.inf
    with pytest.raises(AssertionError, match="NaNs present in moment data"):
        tt.calculate_image_frequency_moments(T.make_cube(_t(pixels)), nmoment=2)
    one = tt.calculate_image_frequency_moments(T.make_cube(_t(pixels)), nmoment=1)
    assert torch.isinf(one["pixels"].data[0, 0, 4, 4])
