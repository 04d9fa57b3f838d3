"""Generate the Taylor-term fixtures tests/golden/taylor_cube.npz and
taylor_skycomp.npz from the REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_taylor.py

The five functions of the reference's image/taylor_terms.py and the four of
sky_component/taylor_terms.py that need no source finder are AST-extracted
and executed with numpy on the datamodels shim, as make_golden.py does.  Only
inputs, settings and outputs are stored -- no reference source text.  The
inputs are rebuilt by tests/taylor_case.py, which the tests share.

  taylor_cube.npz     a 5-channel stokesIQ cube of 17 x 13 pixels at 100 MHz +
                      3 MHz steps: its moments (nmoment 3) about the default
                      and an explicit reference frequency, through the cube
                      and the list function; the cubes rebuilt from them; the
                      decoupled Taylor terms for nmoment 1 and 3 with the
                      pseudo-inverses used; the same for the cube as float32
  taylor_skycomp.npz  three components on 5 channels, stokesIQUV and stokesI:
                      Taylor-term fluxes (nmoment 3), interpolated fluxes
                      (nmoment 2), transposed and gathered fluxes

Every singular value of each coupling matrix must exceed 1e-3 of the largest,
so rcond = 1e-7 cannot truncate differently on another machine.
"""

import os
import sys

import numpy as np
from numpy.polynomial import polynomial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import dm, load_reference, save  # noqa: E402

import taylor_case as T  # noqa: E402


class _Coord:
    """A coordinate as the reference reads one of xarray's: ``.data`` is the
    array, an element has a 0-d ``.data`` of its own."""

    def __init__(self, values):
        self.data = np.asarray(values)

    def __getitem__(self, key):
        return _Coord(self.data[key])


class _CubeView:
    """The shim's Image with such a ``frequency`` (its own ``frequency[chan]``
    is a bare number, which has no numeric ``.data``)."""

    def __init__(self, im):
        self._im = im
        self.frequency = _Coord(im.frequency.data)
        self.image_acc = im.image_acc

    def __getitem__(self, name):
        return self._im[name]


def coupling_pinv(frequency, reference_frequency, nmoment):
    coupling = T.weights(frequency, reference_frequency, nmoment)
    sv = np.linalg.svd(coupling, compute_uv=False)
    assert sv.min() > 1e-3 * sv.max(), sv
    return np.linalg.pinv(coupling, rcond=1e-7), sv.max() / sv.min()


def make_cube(ref):
    cube = T.cube_pixels()
    freq = T.F0 + T.BW * np.arange(T.NCHAN)
    out = dict(cube=cube, frequency=freq, explicit_reference=np.array(T.EXPLICIT_REFERENCE))
    for tag, pixels in (("", cube), ("_f32", cube.astype(np.float32))):
        im, im_list = T.make_cube(pixels), T.make_list(pixels)
        for rtag, rf in (("", None), ("_ref", T.EXPLICIT_REFERENCE)):
            moments = ref["calculate_image_frequency_moments"](im, reference_frequency=rf, nmoment=3)
            listed = ref["calculate_image_list_frequency_moments"](im_list, reference_frequency=rf,
                                                                   nmoment=3)
            assert np.array_equal(moments["pixels"].data, listed["pixels"].data)
            w = moments.image_acc.wcs.wcs
            assert w.ctype[3] == "MOMENT" and w.cunit[3] == "" and w.crval[3] == 0.0
            rebuilt = ref["calculate_image_from_frequency_taylor_terms"](_CubeView(im), moments,
                                                                         reference_frequency=rf)
            relist = ref["calculate_image_list_from_frequency_taylor_terms"](im_list, moments,
                                                                             reference_frequency=rf)
            assert all(np.array_equal(r["pixels"].data[0], rebuilt["pixels"].data[c])
                       for c, r in enumerate(relist))
            assert rebuilt["pixels"].data.dtype == pixels.dtype
            out[f"moments3{rtag}{tag}"] = moments["pixels"].data
            out[f"rebuilt{rtag}{tag}"] = rebuilt["pixels"].data
        for nmoment in (1, 3):
            terms = ref["calculate_frequency_taylor_terms_from_image_list"](im_list, nmoment=nmoment)
            assert len(terms) == nmoment and terms[0].image_acc.wcs.wcs.crval[3] == freq[2]
            out[f"decoupled{nmoment}{tag}"] = np.stack([t["pixels"].data for t in terms])
    for nmoment in (1, 3):
        out[f"pinv{nmoment}"], out[f"cond{nmoment}"] = coupling_pinv(freq, freq[2], nmoment)
    save("taylor_cube.npz", **out)


def make_skycomp(ref):
    out = dict(frequency=T.COMP_FREQUENCY)
    for pol_frame, seed in (("stokesIQUV", 31), ("stokesI", 32)):
        flux = T.components(pol_frame, seed)
        comps = T.make_components(flux, pol_frame)
        terms = ref["calculate_skycomponent_list_taylor_terms"](comps, nmoment=3)
        assert all(t.frequency == T.COMP_FREQUENCY[2] for per in terms for t in per)
        interp = ref["interpolate_skycomponents_frequency"](comps, nmoment=2)
        chans = ref["transpose_skycomponents_to_channels"](comps)
        back = ref["gather_skycomponents_from_channels"](chans)
        out[f"flux_{pol_frame}"] = flux
        out[f"taylor3_{pol_frame}"] = np.array([[t.flux for t in per] for per in terms])
        out[f"interp2_{pol_frame}"] = np.array([c.flux for c in interp])
        out[f"transposed_{pol_frame}"] = np.array([[c.flux for c in per] for per in chans])
        out[f"transposed_frequency_{pol_frame}"] = np.array([[c.frequency for c in per]
                                                             for per in chans])
        out[f"gathered_{pol_frame}"] = np.array([c.flux for c in back])
        assert all(np.array_equal(c.frequency, T.COMP_FREQUENCY) for c in back)
    assert ref["calculate_skycomponent_list_taylor_terms"]([], nmoment=3) == [[]]
    out["pinv3"], out["cond3"] = coupling_pinv(T.COMP_FREQUENCY, T.COMP_FREQUENCY[2], 3)
    x = (T.COMP_FREQUENCY - T.COMP_FREQUENCY[2]) / T.COMP_FREQUENCY[2]
    out["cond_fit2"] = np.array(np.linalg.cond(polynomial.polyvander(x, 1)))
    save("taylor_skycomp.npz", **out)


def main():
    image = load_reference(
        "image/taylor_terms.py",
        ["calculate_image_frequency_moments", "calculate_image_from_frequency_taylor_terms",
         "calculate_image_list_frequency_moments",
         "calculate_image_list_from_frequency_taylor_terms",
         "calculate_frequency_taylor_terms_from_image_list"], {"List": list})
    comp = load_reference(
        "sky_component/taylor_terms.py",
        ["calculate_skycomponent_list_taylor_terms", "interpolate_skycomponents_frequency",
         "transpose_skycomponents_to_channels", "gather_skycomponents_from_channels"],
        {"List": list, "polynomial": polynomial, "SkyComponent": dm.SkyComponent})
    make_cube(image)
    make_skycomp(comp)


if __name__ == "__main__":
    main()
