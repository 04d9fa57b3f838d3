"""GPU tests of the facet gather kernel (csrc/facets.hip through
kernels.gather_facets) and of the scatter / gather functions of
image/gather_scatter.py on device tensors.

Every comparison is bitwise, the signs of zeros included: per output pixel
the kernel adds the facets that cover it in the reference's order, one
rounding per operation in the image's dtype, which is what numpy does in the
reference (tests/golden/facets_*.npz, and the numpy path of the same
functions, which tests/test_facets_cpu.py holds against those fixtures).
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import golden
from ska_sdp_func_python_amd import _lib, image, kernels
from ska_sdp_func_python_amd.image import iterators

import facets_case as C

pytestmark = pytest.mark.gpu

INT = {torch.float64: torch.int64, torch.float32: torch.int32}


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.as_tensor(np.array(a), device=_dev())  # a copy: the cached cases are read-only


def same_bits(got, want):
    """Device tensor against a numpy array (or a tensor) of the same dtype, bit for bit."""
    want = want if isinstance(want, torch.Tensor) else _t(want)
    return got.dtype == want.dtype and got.shape == want.shape and \
        torch.equal(got.contiguous().view(INT[got.dtype]), want.contiguous().view(INT[want.dtype]))


def on_device(images):
    return [C.make_image(_t(im["pixels"].data)) for im in images]


def host_facets(pixels, facets, overlap):
    """The scaled facets of tests/facets_case.py, as separately allocated host images."""
    return C.facet_images(image.image_scatter_facets(C.make_image(pixels), facets=facets,
                                                     overlap=overlap))


# ---- the goldens ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_gather_on_the_device_matches_the_reference_bit_for_bit(name):
    g = golden(f"facets_{name}.npz")
    ny, nx, facets, overlap, taper, dtype = C.CASES[name]
    im = C.make_image(_t(g["pixels"]))
    facet_list = on_device(host_facets(g["pixels"], facets, overlap))
    out = image.image_gather_facets(facet_list, im, facets=facets, overlap=overlap, taper=taper)
    assert out["pixels"].data.is_cuda and same_bits(out["pixels"].data, g["gathered"])
    assert out.image_acc.wcs is im.image_acc.wcs
    flat = image.image_gather_facets(facet_list, im, facets=facets, overlap=overlap, taper=taper,
                                     return_flat=True)
    assert flat["pixels"].data.is_cuda and same_bits(flat["pixels"].data, g["flat"])
    assert same_bits(im["pixels"].data, g["pixels"])  # a template only
    # both outputs of one kernel call
    dy, dx, sy, sx, y0, x0 = iterators.raster_geometry(im, facets, overlap)
    tapers = (None, None) if overlap == 0 else (g["taper_y"], g["taper_x"])
    both = kernels.gather_facets([f["pixels"].data for f in facet_list], facets, (ny, nx), (y0, x0),
                                 (sy, sx), *tapers, normalise=overlap > 0, weights=True)
    assert same_bits(both[0], g["gathered"]) and same_bits(both[1], g["flat"])


# ---- the device path against the numpy path ----------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(ny, nx, facets, overlap, taper, dtype):
    pixels = C.image_pixels(ny, nx, dtype, seed=facets)
    pixels[:, :, ::5, ::3] = -0.0
    facet_list = host_facets(pixels, facets, overlap)
    im = C.make_image(pixels)
    want = image.image_gather_facets(facet_list, im, facets=facets, overlap=overlap, taper=taper)
    flat = image.image_gather_facets(facet_list, im, facets=facets, overlap=overlap, taper=taper,
                                     return_flat=True)
    for a in (pixels, want["pixels"].data, flat["pixels"].data):
        a.setflags(write=False)
    return pixels, facet_list, want["pixels"].data, flat["pixels"].data


# rows that span several x tiles, odd origins (9, 9); rows that cross facet
# boundaries every few pixels (facets of 8 every 6)
SHAPES = [(70, 1100, 2, 9, "linear"), (64, 64, 8, 1, "tukey")]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("ny,nx,facets,overlap,taper", SHAPES)
def test_device_path_equals_numpy_path(ny, nx, facets, overlap, taper, dtype):
    pixels, facet_list, want, want_flat = random_case(ny, nx, facets, overlap, taper, dtype)
    im = C.make_image(_t(pixels))
    dev_list = on_device(facet_list)
    out = image.image_gather_facets(dev_list, im, facets=facets, overlap=overlap, taper=taper)
    assert same_bits(out["pixels"].data, want)
    flat = image.image_gather_facets(dev_list, im, facets=facets, overlap=overlap, taper=taper,
                                     return_flat=True)
    assert same_bits(flat["pixels"].data, want_flat)
    if (ny, nx) == (70, 1100):
        assert iterators.raster_geometry(im, facets, overlap)[4:] == (9, 9)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_strided_views_and_separate_allocations_give_the_same(dtype):
    """Facets scattered from a window of a larger parent keep the parent's
    row and plane strides; their copies are contiguous."""
    ny, nx, facets, overlap = 40, 53, 2, 3
    parent = _t(C.image_pixels(ny + 5, nx + 7, dtype))
    window = parent[..., 2:2 + ny, 3:3 + nx]
    im = C.make_image(window)
    views = image.image_scatter_facets(im, facets=facets, overlap=overlap)
    for v in views:
        data = v["pixels"].data
        assert data.stride() == ((ny + 5) * (nx + 7) * 2, (ny + 5) * (nx + 7), nx + 7, 1)
        assert not data.is_contiguous()
    copies = [C.make_image(v["pixels"].data.clone()) for v in views]
    template = C.make_image(torch.empty((C.NCHAN, 2, ny, nx), dtype=parent.dtype, device=_dev()))
    got_views = image.image_gather_facets(views, template, facets, overlap, taper="quadratic")
    got_copies = image.image_gather_facets(copies, template, facets, overlap, taper="quadratic")
    assert same_bits(got_views["pixels"].data, got_copies["pixels"].data)
    host = C.make_image(window.cpu().numpy())
    want = image.image_gather_facets(image.image_scatter_facets(host, facets, overlap), host,
                                     facets, overlap, taper="quadratic")
    assert same_bits(got_views["pixels"].data, want["pixels"].data)
    # planes that are not evenly spaced are copied by the image function
    odd = []
    for v in copies:
        three = torch.zeros((C.NCHAN, 3) + tuple(v["pixels"].data.shape[2:]), dtype=parent.dtype,
                            device=_dev())
        three[:, ::2] = v["pixels"].data
        odd.append(C.make_image(three[:, ::2]))
    assert odd[0]["pixels"].data.stride(0) != 2 * odd[0]["pixels"].data.stride(1)
    got_odd = image.image_gather_facets(odd, template, facets, overlap, taper="quadratic")
    assert same_bits(got_odd["pixels"].data, want["pixels"].data)


def test_scatter_on_the_device_returns_views():
    ny, nx, facets, overlap = 26, 22, 2, 2
    pixels = _t(C.image_pixels(ny, nx))
    im = C.make_image(pixels)
    subs = image.image_scatter_facets(im, facets=facets, overlap=overlap)
    g = golden("facets_linear_nonsquare.npz")
    for sub, (y, x), crpix in zip(subs, g["origins"], g["crpix"]):
        data = sub["pixels"].data
        assert data.shape == (C.NCHAN, 2, 13, 11) and data.stride() == pixels.stride()
        assert data.data_ptr() == pixels.data_ptr() + 8 * (int(y) * nx + int(x))
        assert data.untyped_storage().data_ptr() == pixels.untyped_storage().data_ptr()
        assert np.array_equal(sub.image_acc.wcs.wcs.crpix, crpix)
    subs[3]["pixels"].data[...] = 7.0
    y, x = (int(v) for v in g["origins"][3])
    assert bool((pixels[..., y:y + 13, x:x + 11] == 7.0).all())
    assert int((pixels == 7.0).sum()) == C.NCHAN * 2 * 13 * 11
    flats = list(iterators.image_raster_iter(im, facets=facets, overlap=overlap, taper="linear",
                                             make_flat=True))
    want = np.outer(g["taper_y"], g["taper_x"])
    assert all(same_bits(f["pixels"].data[1, 0], want) for f in flats)
    blocks = image.image_scatter_channels(im)
    assert blocks[1]["pixels"].data.data_ptr() == pixels.data_ptr() + 8 * 2 * ny * nx
    assert same_bits(image.image_gather_channels(blocks)["pixels"].data, pixels)
    with pytest.raises(ValueError, match="float32 or float64"):
        image.image_scatter_facets(C.make_image(pixels.to(torch.complex64)), facets=2)


def test_gather_past_two_to_the_31_elements():
    """A float32 image of 5 planes of 23171^2 pixels (2.68e9 elements, 10.7 GB)
    gathered from the four views of itself: element offsets of the facets and
    of the output beyond 32 bits; the odd last row and column are uncovered."""
    n, planes = 23171, 5
    pixels = torch.empty((planes, 1, n, n), dtype=torch.float32, device=_dev())
    flat = pixels.view(-1)
    assert flat.numel() > 2 ** 31
    step = 1 << 28
    for a in range(0, flat.numel(), step):
        b = min(a + step, flat.numel())
        flat[a:b] = torch.arange(a, b, device=_dev(), dtype=torch.int64).remainder_(1021).sub_(510)
    im = C.make_image(pixels, pol_frame="stokesI")
    subs = image.image_scatter_facets(im, facets=2)
    assert subs[3]["pixels"].data.data_ptr() == pixels.data_ptr() + 4 * (11585 * n + 11585)
    out = image.image_gather_facets(subs, im, facets=2)["pixels"].data
    assert out.shape == pixels.shape and out.data_ptr() != pixels.data_ptr()
    for p in range(planes):
        assert torch.equal(out[p, 0, :n - 1, :n - 1], pixels[p, 0, :n - 1, :n - 1])
        assert not bool(out[p, 0, n - 1, :].any()) and not bool(out[p, 0, :, n - 1].any())
    tail = (np.arange(planes * n * n - n - 6, planes * n * n - n - 1) % 1021 - 510).astype(np.float32)
    assert np.array_equal(out[-1, 0, n - 2, -6:-1].cpu().numpy(), tail)


# ---- arguments ------------------------------------------------------------------------
def test_gather_facets_refuses_bad_arguments():
    ny, nx, dy, dx = 24, 24, 12, 12
    facet = torch.zeros((2, 2, dy, dx), dtype=torch.float64, device=_dev())
    four = [facet.clone() for _ in range(4)]
    args = (2, (ny, nx), (0, 0), (12, 12))
    with pytest.raises(ValueError, match="3 facets given"):
        kernels.gather_facets(four[:3], *args)
    with pytest.raises(ValueError, match="agree in dtype"):
        kernels.gather_facets(four[:3] + [facet.float()], *args)
    with pytest.raises(ValueError, match="agree in dtype"):
        kernels.gather_facets(four[:3] + [facet[..., :11]], *args)
    with pytest.raises(ValueError, match="device"):
        kernels.gather_facets([f.cpu() for f in four], *args)
    wide = torch.zeros((2, 2, dy, 2 * dx), dtype=torch.float64, device=_dev())
    with pytest.raises(ValueError, match="x stride"):
        kernels.gather_facets(four[:3] + [wide[..., ::2]], *args)
    cube = torch.zeros((2, 3, dy, dx), dtype=torch.float64, device=_dev())
    with pytest.raises(ValueError, match="evenly spaced"):
        kernels.gather_facets(four[:3] + [cube[:, ::2]], *args)
    with pytest.raises(ValueError, match="at least 1"):
        kernels.gather_facets(four, 2, (ny, nx), (0, 0), (12, 0))
    with pytest.raises(ValueError, match="leave the image"):
        kernels.gather_facets(four, 2, (ny, nx), (1, 0), (12, 12))
    with pytest.raises(ValueError, match="float32 or float64"):
        kernels.gather_facets([f.to(torch.float16) for f in four], *args)
    with pytest.raises(ValueError, match="come together"):
        kernels.gather_facets(four, *args, taper_y=np.ones(dy))
    with pytest.raises(ValueError, match="a taper of shape"):
        kernels.gather_facets(four, *args, taper_y=np.ones(dy), taper_x=np.ones(dx + 1))
    many = kernels.GATHER_FACETS_MAX + 1
    with pytest.raises(ValueError, match="1 .. 256 facets"):
        kernels.gather_facets([facet] * (many * many), many, (ny, nx), (0, 0), (12, 12))
    with pytest.raises(ValueError, match="1 .. 256 facets"):
        kernels.gather_facets([], 0, (ny, nx), (0, 0), (12, 12))

    # the library's own checks
    out = torch.full((2, 2, ny, nx), np.nan, dtype=torch.float64, device=_dev())
    ptrs = np.array([f.data_ptr() for f in four], dtype=np.uint64)
    pstride = np.full(4, dy * dx, dtype=np.int64)
    rstride = np.full(4, dx, dtype=np.int64)

    def call(dtype=_lib.SDP_HIP_F64, facets=2, nplanes=4, size=(ny, nx), facet=(dy, dx),
             origin=(0, 0), step=(12, 12), tabs=(ptrs, pstride, rstride), tapers=(None, None),
             outputs=(out, None)):
        host = [ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data)
                for a in tuple(tabs) + tuple(tapers)]
        _lib.call("sdp_hip_gather_facets", dtype, facets, nplanes, *size, *facet, *origin, *step,
                  *host, 0, *[kernels.ptr(o) for o in outputs], kernels.stream(_dev()))

    with pytest.raises(ValueError, match="1 .. 256 facets"):
        call(facets=many)
    with pytest.raises(ValueError, match="1 .. 256 facets"):
        call(facets=0)
    with pytest.raises(ValueError, match="float32 or float64"):
        call(dtype=_lib.SDP_HIP_C64)
    with pytest.raises(ValueError, match="steps between facets"):
        call(step=(12, 0))
    with pytest.raises(ValueError, match="facet size"):
        call(facet=(dy, nx + 1))
    with pytest.raises(ValueError, match="leave the image in y"):
        call(origin=(1, 0))
    with pytest.raises(ValueError, match="leave the image in x"):
        call(origin=(0, -1))
    with pytest.raises(ValueError, match="pixels per side"):
        call(nplanes=0)
    with pytest.raises(ValueError, match="needs an output"):
        call(outputs=(None, None))
    with pytest.raises(ValueError, match="come together"):
        call(tapers=(np.ones(dy), None))
    with pytest.raises(ValueError, match="null pointer"):
        call(tabs=(ptrs, None, rstride))
    with pytest.raises(ValueError, match="null or not aligned"):
        call(tabs=(np.array([ptrs[0], 0, ptrs[2], ptrs[3]], dtype=np.uint64), pstride, rstride))
    with pytest.raises(ValueError, match="null or not aligned"):
        call(tabs=(ptrs + np.uint64(4), pstride, rstride))
    with pytest.raises(ValueError, match="stride is negative"):
        call(tabs=(ptrs, pstride, -rstride))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # a refused call writes nothing
    call()
    torch.cuda.synchronize()
    assert same_bits(out, np.zeros((2, 2, ny, nx)))


def test_gather_facets_honours_a_side_stream():
    g = golden("facets_sixteenfold.npz")
    ny, nx, facets, overlap, taper, dtype = C.CASES["sixteenfold"]
    facet_list = [f["pixels"].data for f in on_device(host_facets(g["pixels"], facets, overlap))]
    dy, dx, sy, sx, y0, x0 = iterators.raster_geometry(C.make_image(g["pixels"]), facets, overlap)
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    out, flat = kernels.gather_facets(facet_list, facets, (ny, nx), (y0, x0), (sy, sx), g["taper_y"],
                                      g["taper_x"], normalise=True, weights=True, stream=side)
    side.synchronize()
    assert same_bits(out, g["gathered"]) and same_bits(flat, g["flat"])
    only = kernels.gather_facet_weights(facets, (C.NCHAN, 2), (dy, dx), (ny, nx), (y0, x0), (sy, sx),
                                        torch.float64, _dev(), g["taper_y"], g["taper_x"])
    assert same_bits(only, g["flat"])
