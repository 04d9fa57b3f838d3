"""fourier_transforms against the reference's own outputs
(tests/golden/fourier_support.npz, fourier_coordinates.npz, written by
make_golden_fourier.py): numpy in, numpy out, bit for bit; torch tensors
through torch.fft and slicing to rounding."""

import numpy as np
import pytest

from conftest import golden


@pytest.fixture(scope="module")
def sup():
    return golden("fourier_support.npz")


@pytest.fixture(scope="module")
def coo():
    return golden("fourier_coordinates.npz")


@pytest.mark.parametrize("tag", ["a2", "a4", "a5"])
def test_fft_ifft_bits(sup, tag):
    from ska_sdp_func_python_amd.fourier_transforms import fft, ifft
    np.testing.assert_array_equal(fft(sup[tag]), sup[f"fft_{tag}"])
    np.testing.assert_array_equal(ifft(sup[tag]), sup[f"ifft_{tag}"])


def test_ifft_of_five_axes_shifts_three():
    """The reference's quirk: ifft of a 5-D array shifts axes 2, 3 and 4 and
    transforms only the last two (the shift of axis 2 is undone again, so it
    still inverts fft)."""
    from ska_sdp_func_python_amd.fourier_transforms import fft, ifft
    a = np.arange(2 * 1 * 3 * 4 * 4, dtype=complex).reshape(2, 1, 3, 4, 4)
    want = np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(a, axes=[2, 3, 4])), axes=[2, 3, 4])
    np.testing.assert_array_equal(ifft(a), want)
    np.testing.assert_allclose(ifft(fft(a)), a, atol=1e-12)


@pytest.mark.parametrize("tag", ["a2", "a4", "a5"])
def test_fft_ifft_of_tensors(sup, tag):
    import torch
    from ska_sdp_func_python_amd.fourier_transforms import fft, ifft
    t = torch.as_tensor(sup[tag])
    for fn, key in ((fft, "fft"), (ifft, "ifft")):
        out = fn(t)
        assert isinstance(out, torch.Tensor)
        np.testing.assert_allclose(out.numpy(), sup[f"{key}_{tag}"], rtol=0, atol=1e-13)


def test_pad_mid(sup):
    import torch
    from ska_sdp_func_python_amd.fourier_transforms import pad_mid
    np.testing.assert_array_equal(pad_mid(sup["pad_in6"], 10), sup["pad_6_10"])
    x = sup["pad_in8"]
    assert pad_mid(x, 8) is x
    np.testing.assert_array_equal(pad_mid(x, 8), sup["pad_8_8"])
    t = torch.as_tensor(sup["pad_in6"])
    np.testing.assert_array_equal(pad_mid(t, 10).numpy(), sup["pad_6_10"])
    assert pad_mid(t, 6) is t
    with pytest.raises(AssertionError):
        pad_mid(sup["pad_in6"], 4)


@pytest.mark.parametrize("n", [9, 10])
@pytest.mark.parametrize("m", [4, 5])
def test_extract_mid(sup, n, m):
    import torch
    from ska_sdp_func_python_amd.fourier_transforms import extract_mid
    np.testing.assert_array_equal(extract_mid(sup[f"mid_in{n}"], m), sup[f"mid_{n}_{m}"])
    np.testing.assert_array_equal(extract_mid(torch.as_tensor(sup[f"mid_in{n}"]), m).numpy(),
                                  sup[f"mid_{n}_{m}"])


@pytest.mark.parametrize("os_", [3, 4])
def test_extract_oversampled(sup, os_):
    import torch
    from ska_sdp_func_python_amd.fourier_transforms import extract_oversampled
    a = sup["over_in"]
    for yf in range(os_):
        for xf in range(os_):
            np.testing.assert_array_equal(extract_oversampled(a, xf, yf, os_, 4),
                                          sup[f"over_{os_}"][yf, xf])
    np.testing.assert_array_equal(
        extract_oversampled(torch.as_tensor(a), 1, 2, os_, 4).numpy(), sup[f"over_{os_}"][2, 1])
    with pytest.raises(AssertionError):
        extract_oversampled(a, os_, 0, os_, 4)
    with pytest.raises(AssertionError):
        extract_oversampled(a, 0, -1, os_, 4)


@pytest.mark.parametrize("n", [7, 8])
def test_coordinates(coo, n):
    from ska_sdp_func_python_amd.fourier_transforms import fft_coordinates as fc
    np.testing.assert_array_equal(np.array(fc.coordinateBounds(n)), coo[f"bounds_{n}"])
    np.testing.assert_array_equal(fc.coordinates(n), coo[f"coordinates_{n}"])
    np.testing.assert_array_equal(fc.coordinates2(n), coo[f"coordinates2_{n}"])
    np.testing.assert_array_equal(np.array(fc.coordinates2Offset(n, 2, 4)), coo[f"offset_{n}"])
    np.testing.assert_array_equal(np.array(fc.coordinates2Offset(n, None, None)),
                                  coo[f"offset_default_{n}"])
    np.testing.assert_array_equal(np.array(fc.coordinates2Offset(n, 2, 4, quadrant=True)),
                                  coo[f"offset_quadrant_{n}"])


def test_w_beam(coo):
    from fourier_cases import W_BEAM_CASES
    from ska_sdp_func_python_amd.fourier_transforms import w_beam
    with np.errstate(invalid="ignore"):
        for tag, (n, fov, w, cx, cy, shift) in W_BEAM_CASES.items():
            got = w_beam(n, fov, w, cx=cx, cy=cy, remove_shift=shift)
            assert got.shape == coo[f"w_beam_{tag}"].shape, tag
            np.testing.assert_array_equal(got, coo[f"w_beam_{tag}"], err_msg=tag)
    assert np.any(coo["w_beam_even_corner"] == 0)     # r2 >= 1 in the corners


def test_grdsf_is_the_one_of_sky_component(coo):
    from ska_sdp_func_python_amd import fourier_transforms
    from ska_sdp_func_python_amd.fourier_transforms import fft_coordinates
    from ska_sdp_func_python_amd.sky_component import operations
    assert fourier_transforms.grdsf is operations.grdsf
    assert fft_coordinates.grdsf is operations.grdsf
    a, b = fourier_transforms.grdsf(coo["grdsf_nu"])
    np.testing.assert_array_equal(a, coo["grdsf_0"])
    np.testing.assert_array_equal(b, coo["grdsf_1"])


def test_names_follow_the_reference():
    from ska_sdp_func_python_amd import fourier_transforms as ft
    from ska_sdp_func_python_amd.fourier_transforms import fft_coordinates, fft_support
    assert fft_support.__all__ == ["extract_mid", "extract_oversampled", "fft", "ifft", "pad_mid"]
    assert fft_coordinates.__all__ == ["coordinates", "grdsf", "w_beam"]
    for name in fft_support.__all__ + fft_coordinates.__all__:
        assert hasattr(ft, name)
