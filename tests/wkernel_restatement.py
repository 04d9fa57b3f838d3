"""The recipe that defines create_awterm_convolutionfunction, composed on the
host from fourier_transforms functions in float64:

    t   = grdsf(|2 * coordinates(N)|)[0]                (ones without use_aaf)
    A_z = w_beam(N, fov, -w_z) * outer(t, t) [* pb[chan, pol]]
    F_z = ifft(pad_mid(A_z, os * N))
    cf[chan, pol, z, iv, iu] = extract_oversampled(F_z, iu - h, iv - h, os, support)

``fns`` names the functions: by default the package's own numpy
fourier_transforms; tests/golden/make_golden_fourier.py passes the
reference's.  Also here: the two images of the fixtures and the geometry they
share with the GPU tests.
"""

import types

import numpy as np

# the fixtures' cases: farfield_npixel, support, oversampling, nw, wstep,
# use_aaf, pb (nchan, npol) or None, the planes stored
CASES = {
    "a": dict(N=18, support=16, os=8, nw=3, wstep=100.0, use_aaf=True, pb=None, planes=(0, 1, 2)),
    "b": dict(N=32, support=8, os=3, nw=1, wstep=1e15, use_aaf=True, pb=None, planes=(0,)),
    "c": dict(N=40, support=12, os=4, nw=3, wstep=500.0, use_aaf=True, pb=(2, 2), planes=(0, 2)),
    "d": dict(N=32, support=16, os=8, nw=3, wstep=10.0, use_aaf=False, pb=None, planes=(0, 1, 2)),
}
IMAGE_NPIXEL, IMAGE_CELL = 64, 0.004
# the end-to-end case (wkernel_e2e.npz): a point source of unit flux at pixel
# [SOURCE_Y, SOURCE_X] seen by 400 visibilities on w planes 10 wavelengths apart
E2E = dict(N=32, support=16, os=8, nw=23, wstep=10.0, nrow=400, uv_cells=20, seed=1,
           frequency=1.0e8, source_y=22, source_x=45, inner=slice(8, 56))
# what of the reference-recipe cf of the end-to-end case the fixture holds (the
# whole of it is 7.6 MB): these w planes, at these offset planes of both axes
E2E_SAMPLE_Z, E2E_SAMPLE_OFFSETS = (0, 11, 22), (0, 4, 8)


def package_functions():
    from ska_sdp_func_python_amd.fourier_transforms import fft_coordinates as fc
    from ska_sdp_func_python_amd.fourier_transforms import fft_support as fs
    return types.SimpleNamespace(coordinates=fc.coordinates, grdsf=fc.grdsf, w_beam=fc.w_beam,
                                 pad_mid=fs.pad_mid, ifft=fs.ifft,
                                 extract_oversampled=fs.extract_oversampled)


def case_image(case):
    """The template image of a fixture case: 64 x 64 pixels of 0.004 rad,
    stokesI, or 2 channels of linearnp (2 polarisations) for the case with a
    primary beam."""
    from ska_sdp_func_python_amd import datamodels as dm
    pb = CASES[case]["pb"]
    if pb is None:
        return dm.create_image(IMAGE_NPIXEL, IMAGE_CELL, dm.SkyCoord(0.5, -0.7), frequency=1.0e8,
                               channel_bandwidth=2.0e6)
    return dm.create_image(IMAGE_NPIXEL, IMAGE_CELL, dm.SkyCoord(0.5, -0.7),
                           polarisation_frame=dm.PolarisationFrame("linearnp"), frequency=1.0e8,
                           channel_bandwidth=2.0e6, nchan=pb[0])


def case_pb(case):
    """A smooth complex primary beam [nchan, npol, N, N] for the case, or None:
    an off-centre Gaussian with a phase gradient, different in every plane."""
    c = CASES[case]
    if c["pb"] is None:
        return None
    nchan, npol = c["pb"]
    n = c["N"]
    y, x = (np.mgrid[0:n, 0:n] - n // 2) / n
    out = np.zeros((nchan, npol, n, n), complex)
    for ch in range(nchan):
        for p in range(npol):
            k = 1 + ch * npol + p
            amp = np.exp(-((x - 0.02 * k) ** 2 + (y + 0.03 * k) ** 2) / (0.18 + 0.02 * k))
            out[ch, p] = amp * np.exp(1j * (0.4 * k * x - 0.3 * y + 0.1 * k))
    return out


def e2e_image():
    from ska_sdp_func_python_amd import datamodels as dm
    return dm.create_image(IMAGE_NPIXEL, IMAGE_CELL, dm.SkyCoord(0.5, -0.7),
                           frequency=E2E["frequency"], channel_bandwidth=2.0e6)


def e2e_visibility(im, uvw, vis):
    """The Visibility of the end-to-end case: ``uvw`` [nrow, 1, 3] in metres,
    ``vis`` [nrow, 1, 1, 1], unit weights, at the image's phase centre."""
    from ska_sdp_func_python_amd import datamodels as dm
    shape = vis.shape
    return dm.Visibility.constructor(
        frequency=np.array([E2E["frequency"]]), channel_bandwidth=np.array([2.0e6]),
        phasecentre=im.image_acc.phasecentre, uvw=uvw, time=np.arange(shape[0], dtype=float),
        vis=vis, weight=np.ones(shape), flags=np.zeros(shape, int), baselines=np.array([[0, 1]]),
        polarisation_frame=dm.PolarisationFrame("stokesI"), imaging_weight=np.ones(shape))


def extract(fns, parent, xf, yf, os, support):
    """extract_oversampled, its slice arithmetic carried on to negative offsets."""
    if xf >= 0 and yf >= 0:
        return fns.extract_oversampled(parent, xf, yf, os, support)
    c0 = parent.shape[0] // 2 - os * (support // 2)
    my, mx = c0 - yf, c0 - xf
    assert my >= 0 and mx >= 0
    return os * os * parent[my:my + os * support:os, mx:mx + os * support:os]


def farfield(fns, n, fov, w, use_aaf, pb_plane=None):
    a = fns.w_beam(n, fov, -w)
    if use_aaf:
        t = fns.grdsf(np.abs(2 * fns.coordinates(n)))[0]
        a = a * np.outer(t, t)
    if pb_plane is not None:
        a = a * pb_plane
    return a


def recipe(n, fov, ws, os, support, use_aaf=True, pb=None, fns=None):
    """cf [nb, len(ws), nd, nd, support, support] complex128 for the plane
    values ``ws``; nb is 1 without ``pb``, else the planes of ``pb`` [nb, N, N]."""
    fns = fns or package_functions()
    h = os // 2
    nd = 2 * h + 1
    beams = [None] if pb is None else list(pb)
    cf = np.zeros((len(beams), len(ws), nd, nd, support, support), complex)
    for b, beam in enumerate(beams):
        for z, w in enumerate(ws):
            parent = fns.ifft(fns.pad_mid(farfield(fns, n, fov, w, use_aaf, beam), os * n))
            for iv in range(nd):
                for iu in range(nd):
                    cf[b, z, iv, iu] = extract(fns, parent, iu - h, iv - h, os, support)
    return cf


def restate_awterm(im, nw=1, wstep=1e15, oversampling=8, support=16, use_aaf=True,
                   farfield_npixel=None, pb=None, normalise=True, fns=None):
    """The pixels [nchan, npol, nw, nd, nd, support, support] of
    create_awterm_convolutionfunction's cf, from the recipe."""
    nchan, _, _, nx = im["pixels"].data.shape
    n = farfield_npixel
    if n is None:
        n = max(support + 2, 32)
        n += n % 2
    fov = nx * float(np.deg2rad(abs(im.image_acc.wcs.wcs.cdelt[1])))
    ws = [(z - nw // 2) * float(wstep) for z in range(nw)]
    h = oversampling // 2
    if pb is None:
        cf = recipe(n, fov, ws, oversampling, support, use_aaf, None, fns)
        npol = im["pixels"].data.shape[1]
        cf = np.broadcast_to(cf[0], (nchan, npol) + cf.shape[1:]).copy()
    else:
        cf = recipe(n, fov, ws, oversampling, support, use_aaf, pb.reshape((-1,) + pb.shape[2:]),
                    fns).reshape(pb.shape[:2] + (nw, 2 * h + 1, 2 * h + 1, support, support))
    if normalise:
        cf = cf / np.sum(np.real(cf[0, 0, nw // 2, h, h]))
    return cf
