"""create_awterm_convolutionfunction / sdp_hip_wkernel_create on the GPU.

Parity: against the recipe as direct sums in numpy.longdouble (cf_ld of
tests/golden/wkernel_*_ld.npz), within 4 S, where S is the error that the
recipe in float64 has of itself (make_golden_fourier.py): the device's
sincospi, its FMAs and its summation order are independent roundings of the
size S already contains.  Structure: equal bits wherever the same sample is
computed twice.  End to end: a point source through invert_awprojection.
"""

import numpy as np
import pytest

import wkernel_restatement as W
from conftest import golden

pytestmark = pytest.mark.gpu


def _create(case, im=None, **kw):
    from ska_sdp_func_python_amd.grid_data import create_awterm_convolutionfunction
    c = W.CASES[case]
    args = dict(nw=c["nw"], wstep=c["wstep"], oversampling=c["os"], support=c["support"],
                use_aaf=c["use_aaf"], farfield_npixel=c["N"], pb=W.case_pb(case), normalise=False)
    args.update(kw)
    return create_awterm_convolutionfunction(im if im is not None else W.case_image(case), **args)


@pytest.fixture(scope="module")
def created():
    """(gcf, cf) of every fixture case, not normalised, from numpy images."""
    return {case: _create(case) for case in W.CASES}


def _device_planes(case, ws, pb=True):
    """kernels.wkernel_create for the case's geometry at the plane values ws."""
    import torch
    from ska_sdp_func_python_amd import kernels
    from ska_sdp_func_python_amd.fourier_transforms import coordinates, grdsf
    c = W.CASES[case]
    dev = torch.device("cuda:0")
    fov = float(golden(f"wkernel_{case}.npz")["fov"])
    taper = None
    if c["use_aaf"]:
        taper = torch.as_tensor(grdsf(np.abs(2 * coordinates(c["N"])))[0], device=dev)
    beam = W.case_pb(case) if pb else None
    if beam is not None:
        beam = torch.as_tensor(beam.reshape(-1, c["N"], c["N"]), device=dev)
    w = torch.as_tensor(list(ws), dtype=torch.float64, device=dev)
    return kernels.wkernel_create(c["N"], c["os"], c["support"], w, fov, taper=taper, pb=beam)


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_parity_with_longdouble_sums(created, case):
    g = golden(f"wkernel_{case}.npz")
    ld = golden(f"wkernel_{case}_ld.npz")["cf_ld"]
    c = W.CASES[case]
    gcf, cf = created[case]
    px = cf["pixels"].data
    nd = 2 * (c["os"] // 2) + 1
    nchan, npol = (1, 1) if c["pb"] is None else c["pb"]
    assert isinstance(px, np.ndarray) and px.dtype == np.complex128
    assert px.shape == (nchan, npol, c["nw"], nd, nd, c["support"], c["support"])
    dev = px[:, :, list(c["planes"])].reshape(ld.shape)
    err = np.abs(dev - ld).max() / np.abs(ld).max()
    s = float(g["S"])
    print(f"case {case}: device error {err:.3e} = {err / s:.2f} S (S = {s:.3e})")
    assert err <= 4 * s
    assert cf.convolutionfunction_acc.cf_wcs.wcs.crpix[4] == c["nw"] // 2 + 1


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_grid_correction_and_normalisation(created, case):
    c = W.CASES[case]
    gcf = created[case][0]["pixels"].data
    want = golden("wkernel_e2e.npz")["gcf"][0, 0] if c["use_aaf"] else np.ones((64, 64))
    assert gcf.dtype == np.float64
    np.testing.assert_array_equal(gcf, np.broadcast_to(want, gcf.shape))
    _, cf = _create(case, normalise=True)
    h = c["os"] // 2
    total = np.sum(np.real(cf["pixels"].data[0, 0, c["nw"] // 2, h, h]))
    s = float(golden(f"wkernel_{case}.npz")["S"])
    print(f"case {case}: |sum - 1| = {abs(total - 1):.3e} = {abs(total - 1) / s:.2f} S")
    assert abs(total - 1) <= 4 * s


def test_rerun_has_equal_bits():
    import torch
    a = _device_planes("c", [-500.0, 0.0, 500.0])
    b = _device_planes("c", [-500.0, 0.0, 500.0])
    assert a.shape == (4, 3, 5, 5, 12, 12)
    assert torch.equal(a.view(torch.float64), b.view(torch.float64))


@pytest.mark.parametrize("case", ["a", "c"])
def test_plane_alone_split_and_batch_have_equal_bits(case):
    import torch
    c = W.CASES[case]
    ws = [(z - 2) * c["wstep"] for z in range(5)]
    batch = _device_planes(case, ws).view(torch.float64)
    for z in (0, 3):
        alone = _device_planes(case, [ws[z]]).view(torch.float64)
        assert torch.equal(alone[:, 0], batch[:, z]), z
    first = _device_planes(case, ws[:2]).view(torch.float64)
    second = _device_planes(case, ws[2:]).view(torch.float64)
    assert torch.equal(torch.cat([first, second], dim=1), batch)
    if c["pb"] is not None:     # and a beam's planes do not depend on the other beams
        one = torch.as_tensor(W.case_pb(case)[1, 0][None], device="cuda:0")
        from ska_sdp_func_python_amd import kernels
        from ska_sdp_func_python_amd.fourier_transforms import coordinates, grdsf
        taper = torch.as_tensor(grdsf(np.abs(2 * coordinates(c["N"])))[0], device="cuda:0")
        w = torch.as_tensor(ws, dtype=torch.float64, device="cuda:0")
        got = kernels.wkernel_create(c["N"], c["os"], c["support"], w,
                                     float(golden(f"wkernel_{case}.npz")["fov"]), taper=taper,
                                     pb=one).view(torch.float64)
        assert torch.equal(got[0], batch[2])


def test_chunked_call_keeps_plane_bits():
    """130 planes of 256 pixels are more than the library holds far fields
    for at a time (117): the planes of its second chunk, and tiles beyond the
    first in both products (288 = 4.5 tiles of samples), have the bits of
    planes computed alone."""
    import torch
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    ws = [(z - 65) * 50.0 for z in range(130)]
    w = torch.as_tensor(ws, dtype=torch.float64, device=dev)
    cf = kernels.wkernel_create(256, 8, 32, w, 0.2)
    assert cf.shape == (1, 130, 9, 9, 32, 32)
    for z in (3, 116, 117, 129):
        alone = kernels.wkernel_create(256, 8, 32, w[z:z + 1].clone(), 0.2)
        assert torch.equal(alone[0, 0].view(torch.float64), cf[0, z].view(torch.float64)), z
    # w = 0 is plane 65; its centre kernel sums to 1 (no taper: a box's transform)
    total = float(cf[0, 65, 4, 4].real.sum())
    assert abs(total - 1) < 1e-3


@pytest.mark.parametrize("case", ["a", "c"])       # oversampling 8 and 4
def test_end_offset_planes_are_shifted_copies(created, case):
    cf = created[case][1]["pixels"].data
    top = 2 * (W.CASES[case]["os"] // 2)
    np.testing.assert_array_equal(cf[:, :, :, :, top, :, 1:], cf[:, :, :, :, 0, :, :-1])
    np.testing.assert_array_equal(cf[:, :, :, top, :, 1:, :], cf[:, :, :, 0, :, :-1, :])


def test_results_live_where_the_image_lives(created):
    import torch
    im = W.case_image("c")
    im["pixels"].data = torch.zeros(im["pixels"].data.shape, dtype=torch.float64, device="cuda:0")
    gcf_d, cf_d = _create("c", im=im)
    gcf_h, cf_h = created["c"]
    for dev_px, host_px in ((gcf_d["pixels"].data, gcf_h["pixels"].data),
                            (cf_d["pixels"].data, cf_h["pixels"].data)):
        assert isinstance(dev_px, torch.Tensor) and dev_px.is_cuda
        assert isinstance(host_px, np.ndarray)
        np.testing.assert_array_equal(dev_px.cpu().numpy(), host_px)
    # without a beam the [nchan, npol] axes of a device result are an expand
    im1 = W.case_image("a")
    im1["pixels"].data = torch.zeros((3, 1, 64, 64), dtype=torch.float64, device="cuda:0")
    _, cf3 = _create("a", im=im1)
    px = cf3["pixels"].data
    assert px.shape[:2] == (3, 1) and px.stride(0) == 0
    np.testing.assert_array_equal(px[2, 0].cpu().numpy(), created["a"][1]["pixels"].data[0, 0])


def test_pswf_is_the_single_plane_case():
    from ska_sdp_func_python_amd.grid_data import (create_awterm_convolutionfunction,
                                                   create_pswf_convolutionfunction)
    im = W.case_image("a")
    gcf, cf = create_pswf_convolutionfunction(im, oversampling=4, support=6)
    gcf2, cf2 = create_awterm_convolutionfunction(im, nw=1, oversampling=4, support=6)
    assert cf["pixels"].data.shape == (1, 1, 1, 5, 5, 6, 6)
    np.testing.assert_array_equal(cf["pixels"].data, cf2["pixels"].data)
    np.testing.assert_array_equal(gcf["pixels"].data, gcf2["pixels"].data)
    want = W.restate_awterm(im, 1, 1e15, 4, 6)
    assert np.abs(cf["pixels"].data - want).max() <= 1e-14 * np.abs(want).max()


def test_wrapper_refuses_bad_operands():
    import torch
    from ska_sdp_func_python_amd import kernels
    dev = torch.device("cuda:0")
    w = torch.zeros(3, dtype=torch.float64, device=dev)
    for bad in (dict(w=w.cpu()), dict(w=w.float()), dict(w=torch.zeros(6, dtype=torch.float64,
                                                                       device=dev)[::2]),
                dict(support=7), dict(npixel=17), dict(npixel=8), dict(oversampling=0),
                dict(taper=torch.ones(17, dtype=torch.float64, device=dev)),
                dict(pb=torch.ones((2, 18, 18), dtype=torch.complex64, device=dev)),
                dict(pb=torch.ones((18, 18), dtype=torch.complex128, device=dev))):
        args = dict(npixel=18, oversampling=8, support=16, w=w, field_of_view=0.25)
        args.update(bad)
        with pytest.raises(ValueError):
            kernels.wkernel_create(**args)


def test_point_source_end_to_end():
    """A unit point source at pixel [22, 45], 400 visibilities with |w| <= 100
    wavelengths on planes 10 apart: invert_awprojection with the created
    (gcf, cf) against the same with the reference-recipe (gcf, cf) and against
    the direct-sum dirty image d.  With the recipe's sign or orientation wrong
    the error against d is 1.1, not 0.05."""
    from ska_sdp_func_python_amd import datamodels as dm
    from ska_sdp_func_python_amd.grid_data import (convolution_mapping_visibility,
                                                   create_awterm_convolutionfunction)
    from ska_sdp_func_python_amd.imaging.base import invert_awprojection
    g = golden("wkernel_e2e.npz")
    E = W.E2E
    im = W.e2e_image()
    vis = W.e2e_visibility(im, g["uvw"], g["vis"])
    kw = dict(nw=E["nw"], wstep=E["wstep"], oversampling=E["os"], support=E["support"],
              farfield_npixel=E["N"])
    gcf, cf = create_awterm_convolutionfunction(im, **kw)

    # the reference-recipe pair: the fixture's gcf, and the cf recomputed on the
    # host (the fixture holds samples of it: the whole is too large to commit)
    ref_px = W.restate_awterm(im, E["nw"], E["wstep"], E["os"], E["support"], True, E["N"])
    offs = list(W.E2E_SAMPLE_OFFSETS)
    np.testing.assert_array_equal(ref_px[0, 0][list(W.E2E_SAMPLE_Z)][:, offs][:, :, offs],
                                  g["cf_sample"])
    ref_cf = dm.ConvolutionFunction.constructor(ref_px, cf.convolutionfunction_acc.cf_wcs,
                                                dm.PolarisationFrame("stokesI"))
    ref_gcf = im.copy(deep=True)
    ref_gcf["pixels"].data = g["gcf"].copy()
    np.testing.assert_array_equal(gcf["pixels"].data, g["gcf"])

    made, sumwt = invert_awprojection(vis, im, gcfcf=lambda _im: (gcf, cf))
    want, sumwt_ref = invert_awprojection(vis, im, gcfcf=lambda _im: (ref_gcf, ref_cf))
    a = np.asarray(made["pixels"].data)[0, 0]
    b = np.asarray(want["pixels"].data)[0, 0]
    np.testing.assert_array_equal(sumwt, sumwt_ref)
    src = (E["source_y"], E["source_x"])
    assert np.unravel_index(np.argmax(a), a.shape) == src
    assert np.unravel_index(np.argmax(b), b.shape) == src
    assert a[src] > 0.99
    rel = np.sqrt(np.mean((a - b) ** 2) / np.mean(b ** 2))
    np.testing.assert_allclose(b, g["image_host"], rtol=0, atol=1e-10)
    inner = E["inner"]
    d = g["d"][inner, inner]
    err = np.sqrt(np.mean((a[inner, inner] - d) ** 2) / np.mean(d ** 2))
    print(f"created vs reference-recipe image: {rel:.3e}; against d: {err:.4f} "
          f"(E_host {float(g['E_host']):.4f})")
    assert rel <= 1e-10
    assert err <= 1.05 * float(g["E_host"])

    # offsets that round to +h use the (2 h + 1)-th offset plane: no overflow
    gd = dm.create_griddata_from_image(im)
    _, pdu, _, pdv, pwc, _ = convolution_mapping_visibility(vis, gd, 0, cf)
    top = 2 * (E["os"] // 2)
    frac = float(((pdu == top).sum() + (pdv == top).sum()).item()) / (2 * pdu.numel())
    assert 0.03 < frac < 0.10
    assert int(pwc.min()) >= 0 and int(pwc.max()) <= E["nw"] - 1
