"""Generate the fourier_transforms and w-kernel fixtures from the REFERENCE's
own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_fourier.py

The functions of the reference's fourier_transforms/fft_support.py (its branch
without pyfftw) and fft_coordinates.py are AST-extracted and executed with
numpy, as make_golden.py does.  Only inputs and outputs are stored -- no
reference source text.

  fourier_support.npz      fft / ifft (2, 4 and 5 axes), pad_mid, extract_mid,
                           extract_oversampled: inputs and outputs
  fourier_coordinates.npz  coordinateBounds, coordinates, coordinates2,
                           coordinates2Offset, w_beam, grdsf
  wkernel_<case>.npz       the convolution function of tests/wkernel_restatement
                           .recipe run with the reference's functions (cf, not
                           normalised) for the cases a - d there, with S
  wkernel_<case>_ld.npz    cf_ld: the same recipe as direct sums in
                           numpy.longdouble, rounded to float64 on the store
  wkernel_<case>_direct.npz  cf_direct: the pruned sums that csrc/wkernel.hip
                           evaluates, in numpy float64
  wkernel_e2e.npz          a point source seen through 400 visibilities on 23
                           w planes: uvw, vis, the grid correction, samples of
                           the reference-recipe cf, the direct-sum dirty image d
                           and E_host, the error of the reference's
                           invert_awprojection with that cf against d

S = max(|cf - cf_ld|, |cf_direct - cf_ld|) / max|cf_ld| is the error that the
recipe in float64 has of itself: the device result is held to 4 S.  The three
arrays of a case are three files because one file may hold 1 MiB at the most;
for the same reason the 7.6 MB cf of the end-to-end case is not stored: the
GPU test recomputes it with tests/wkernel_restatement (which the CPU tests pin
to cf of the cases a - d bit for bit) and checks it against the stored samples.
"""

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.modules["pyfftw"] = None

from make_golden import _aw_reference, dm, load_reference, save  # noqa: E402

import wkernel_restatement as W  # noqa: E402
from fourier_cases import W_BEAM_CASES  # noqa: E402

LD = np.longdouble
CLD = np.clongdouble


def reference_functions():
    fs = load_reference("fourier_transforms/fft_support.py",
                        ["fft", "ifft", "pad_mid", "extract_mid", "extract_oversampled"],
                        {"pyfftw_exists": False, "pyfftw": None})
    fc = load_reference("fourier_transforms/fft_coordinates.py",
                        ["coordinateBounds", "coordinates", "coordinates2", "coordinates2Offset",
                         "grdsf", "w_beam"])
    names = {k: v for ns in (fs, fc) for k, v in ns.items() if callable(v)}
    return types.SimpleNamespace(**names)


def _complex(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def make_support():
    R = reference_functions()
    rng = np.random.default_rng(21)
    out = {}
    for tag, shape in (("a2", (6, 8)), ("a4", (2, 1, 6, 8)), ("a5", (2, 1, 2, 6, 8))):
        a = _complex(rng, shape)
        out[tag] = a
        out[f"fft_{tag}"] = R.fft(a)
        out[f"ifft_{tag}"] = R.ifft(a)
    out["pad_in6"] = _complex(rng, (2, 6, 6))
    out["pad_6_10"] = R.pad_mid(out["pad_in6"], 10)
    out["pad_in8"] = _complex(rng, (8, 8))
    out["pad_8_8"] = R.pad_mid(out["pad_in8"], 8)
    for n in (9, 10):
        out[f"mid_in{n}"] = _complex(rng, (2, n, n))
        for m in (4, 5):
            out[f"mid_{n}_{m}"] = R.extract_mid(out[f"mid_in{n}"], m)
    out["over_in"] = _complex(rng, (24, 24))
    for os_ in (3, 4):
        out[f"over_{os_}"] = np.array([[R.extract_oversampled(out["over_in"], xf, yf, os_, 4)
                                        for xf in range(os_)] for yf in range(os_)])
    save("fourier_support.npz", **out)


def make_coordinates():
    R = reference_functions()
    out = {}
    for n in (7, 8):
        out[f"bounds_{n}"] = np.array(R.coordinateBounds(n))
        out[f"coordinates_{n}"] = R.coordinates(n)
        out[f"coordinates2_{n}"] = R.coordinates2(n)
        out[f"offset_{n}"] = np.array(R.coordinates2Offset(n, 2, 4))
        out[f"offset_default_{n}"] = np.array(R.coordinates2Offset(n, None, None))
        out[f"offset_quadrant_{n}"] = np.array(R.coordinates2Offset(n, 2, 4, quadrant=True))
    with np.errstate(invalid="ignore"):
        for tag, (n, fov, w, cx, cy, shift) in W_BEAM_CASES.items():
            out[f"w_beam_{tag}"] = R.w_beam(n, fov, w, cx=cx, cy=cy, remove_shift=shift)
    assert np.any(out["w_beam_even_corner"] == 0) and np.any(out["w_beam_odd_corner"] == 0)
    nu = np.linspace(-1.2, 1.2, 49)
    out["grdsf_nu"] = nu
    out["grdsf_0"], out["grdsf_1"] = R.grdsf(nu)
    save("fourier_coordinates.npz", **out)


# ---------------------------------------------------------------------------
def _grdsf_ld(nu):
    """The spheroidal function's value (first result of grdsf) in longdouble."""
    from ska_sdp_func_python_amd.sky_component.operations import _GRDSF_P, _GRDSF_Q
    nu = np.abs(nu.astype(LD))
    part = (nu >= 0.75).astype(int)
    nuend = np.where(part == 1, LD(1.0), LD(0.75))
    d = nu**2 - nuend**2
    top = sum(_GRDSF_P[part, k].astype(LD) * d**k for k in range(_GRDSF_P.shape[1]))
    bot = sum(_GRDSF_Q[part, k].astype(LD) * d**k for k in range(_GRDSF_Q.shape[1]))
    return np.where(nu > 1, LD(0), top / bot)


def sample_offsets(os_, support):
    """j = os (k - support / 2) - (i - h) for row i * support + k."""
    h = os_ // 2
    i, k = np.divmod(np.arange((2 * h + 1) * support), support)
    return os_ * (k - support // 2) - (i - h)


def _to_cf_layout(f, nd, support):
    return f.reshape(nd, support, nd, support).transpose(0, 2, 1, 3)


def recipe_ld(n, fov, ws, os_, support, use_aaf, pb):
    """The recipe as direct sums in longdouble; the w beam's phase in the form
    without cancellation, 2 pi w r2 / (1 + sqrt(1 - r2))."""
    pi = 4 * np.arctan(LD(1))
    nd = 2 * (os_ // 2) + 1
    npad = os_ * n
    x = np.arange(n) - n // 2
    m = (sample_offsets(os_, support)[:, None] * x[None, :]) % npad
    ang = 2 * pi * m.astype(LD) / LD(npad)
    e = (np.cos(ang) + 1j * np.sin(ang)).astype(CLD)
    c = x.astype(LD) / LD(n)
    r2 = LD(fov) ** 2 * (c[:, None] ** 2 + c[None, :] ** 2)
    inside = r2 < 1
    chirp = np.where(inside, r2 / (1 + np.sqrt(np.where(inside, 1 - r2, LD(0)))), LD(0))
    t = _grdsf_ld(np.abs(2 * c)) if use_aaf else np.ones(n, LD)
    beams = [None] if pb is None else list(pb)
    out = np.zeros((len(beams), len(ws), nd, nd, support, support), CLD)
    for b, beam in enumerate(beams):
        for z, w in enumerate(ws):
            ph = 2 * pi * LD(w) * chirp
            a = np.where(inside, np.cos(ph) + 1j * np.sin(ph), 0).astype(CLD) * np.outer(t, t)
            if beam is not None:
                a = a * beam.astype(CLD)
            out[b, z] = _to_cf_layout(e @ a @ e.T / LD(n) ** 2, nd, support)
    return out


def recipe_direct(R, n, fov, ws, os_, support, use_aaf, pb):
    """The pruned sums in float64: the reference's far field between twiddles
    whose exponent is reduced as an integer."""
    nd = 2 * (os_ // 2) + 1
    npad = os_ * n
    x = np.arange(n) - n // 2
    m = (sample_offsets(os_, support)[:, None] * x[None, :]) % npad
    m = np.where(2 * m > npad, m - npad, m)
    ang = 2 * np.pi * (m / npad)
    e = np.cos(ang) + 1j * np.sin(ang)
    beams = [None] if pb is None else list(pb)
    out = np.zeros((len(beams), len(ws), nd, nd, support, support), complex)
    for b, beam in enumerate(beams):
        for z, w in enumerate(ws):
            a = W.farfield(R, n, fov, w, use_aaf, beam)
            out[b, z] = _to_cf_layout(e @ a @ e.T / n**2, nd, support)
    return out


def make_wkernel():
    R = reference_functions()
    for case, c in W.CASES.items():
        im = W.case_image(case)
        fov = im["pixels"].data.shape[3] * float(np.deg2rad(abs(im.image_acc.wcs.wcs.cdelt[1])))
        ws = [(z - c["nw"] // 2) * c["wstep"] for z in c["planes"]]
        pb = W.case_pb(case)
        flat = None if pb is None else pb.reshape((-1,) + pb.shape[2:])
        args = (c["N"], fov, ws, c["os"], c["support"], c["use_aaf"], flat)
        cf = W.recipe(*args, fns=R)
        cf_ld = recipe_ld(*args)
        cf_direct = recipe_direct(R, *args)
        peak = np.abs(cf_ld).max()
        s = float(max(np.abs(cf - cf_ld).max(), np.abs(cf_direct - cf_ld).max()) / peak)
        print(f"case {case}: S = {s:.3e} (fft {np.abs(cf - cf_ld).max() / peak:.3e}, direct "
              f"{np.abs(cf_direct - cf_ld).max() / peak:.3e})")
        save(f"wkernel_{case}.npz", cf=cf, S=np.array(s), fov=np.array(fov), w=np.array(ws))
        save(f"wkernel_{case}_ld.npz", cf_ld=cf_ld.astype(complex))
        save(f"wkernel_{case}_direct.npz", cf_direct=cf_direct)


# ---------------------------------------------------------------------------
def make_e2e():
    R = reference_functions()
    ref = _aw_reference()
    E = W.E2E
    im = W.e2e_image()
    npix, cell = W.IMAGE_NPIXEL, W.IMAGE_CELL
    rng = np.random.default_rng(E["seed"])
    du = 1.0 / (npix * cell)
    uvw_l = np.zeros((E["nrow"], 1, 3))
    uvw_l[..., :2] = rng.uniform(-E["uv_cells"] * du, E["uv_cells"] * du, (E["nrow"], 1, 2))
    uvw_l[..., 2] = E["wstep"] * rng.integers(-10, 11, (E["nrow"], 1))
    # pixel x lies at l = (x - nx / 2) * cdelt_x with cdelt_x = -cell
    l = -(E["source_x"] - npix // 2) * cell
    m = (E["source_y"] - npix // 2) * cell
    n = np.sqrt(1 - l * l - m * m)
    vis = np.exp(-2j * np.pi * (uvw_l[..., 0] * l + uvw_l[..., 1] * m + uvw_l[..., 2] * (n - 1)))
    vis = vis[..., None, None]
    uvw = uvw_l * (dm.C_M_S / E["frequency"])
    # the direct sum: the image that the visibilities define, w term included
    ls = -(np.arange(npix) - npix // 2) * cell
    ms = (np.arange(npix) - npix // 2) * cell
    nn = np.sqrt(1 - ls[None, :] ** 2 - ms[:, None] ** 2)
    d = np.zeros((npix, npix))
    for r in range(E["nrow"]):
        u, v, w = uvw_l[r, 0]
        d += np.real(vis[r, 0, 0, 0] * np.exp(2j * np.pi * (u * ls[None, :] + v * ms[:, None]
                                                            + w * (nn - 1))))
    d /= E["nrow"]

    cfp = W.restate_awterm(im, E["nw"], E["wstep"], E["os"], E["support"], True, E["N"], None,
                           True, fns=R)
    from ska_sdp_func_python_amd.grid_data import convolution_functions as C
    cf = dm.ConvolutionFunction.constructor(
        cfp, C.cf_wcs_for_image(im, E["nw"], E["wstep"], E["os"], E["support"]),
        dm.PolarisationFrame("stokesI"))
    tg = R.grdsf(np.abs(2 * R.coordinates(npix)))[0]
    gcf = im.copy(deep=True)
    gcf["pixels"].data = np.broadcast_to(1 / np.outer(tg, tg), (1, 1, npix, npix)).copy()
    v = W.e2e_visibility(im, uvw, vis)
    dirty, sumwt = ref["invert_awprojection"](v, im, gcfcf=lambda _im: (gcf, cf))
    img = np.asarray(dirty["pixels"].data)[0, 0]
    inner = E["inner"]
    e_host = float(np.sqrt(np.mean((img[inner, inner] - d[inner, inner]) ** 2)
                           / np.mean(d[inner, inner] ** 2)))
    peak = np.unravel_index(np.argmax(img), img.shape)
    print(f"E_host {e_host:.4f}, peak {img.max():.4f} at {peak}, d peak {d.max():.4f} at "
          f"{np.unravel_index(np.argmax(d), d.shape)}")
    # conditions on the input, not on the code under test
    assert e_host < 0.1, e_host
    assert peak == (E["source_y"], E["source_x"]) and img.max() > 0.99, (peak, img.max())
    offs = list(W.E2E_SAMPLE_OFFSETS)
    sample = cfp[0, 0][list(W.E2E_SAMPLE_Z)][:, offs][:, :, offs]
    save("wkernel_e2e.npz", uvw=uvw, vis=vis, gcf=gcf["pixels"].data, cf_sample=sample, d=d,
         E_host=np.array(e_host), image_host=img)


if __name__ == "__main__":
    names = sys.argv[1:] or ["support", "coordinates", "wkernel", "e2e"]
    for name in names:
        globals()[f"make_{name}"]()
