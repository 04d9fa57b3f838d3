"""Generate the imaging-helper fixtures tests/golden/imghelp_*.npz from the
REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_imghelp.py

The four functions of the reference's imaging/imaging_helpers.py and
create_image_from_visibility, advise_wide_field, rad_deg_arcsec and
visibility_recentre of its imaging/base.py are AST-extracted and executed
with numpy on the datamodels shim, as make_golden.py does.  Only outputs are
stored -- no reference source text; the inputs are rebuilt from seeds and
settings by tests/imghelp_case.py, which the tests share.

astropy is absent: ``units`` is a stand-in that serves ``x * units.Hz`` and
``.to(units.Hz).value``.  ``sys.modules["pyfftw"] = None`` makes the import in
advise_wide_field fail, so its fallback branch runs whatever is installed.
Pixels are float64 throughout: numpy 1 and numpy 2 promote a float32 array
times a float64 scalar differently.

  imghelp_sum.npz        sum_invert_results and sum_predict_results
  imghelp_threshold.npz  threshold_list, one value per case
  imghelp_image.npz      create_image_from_visibility: shape, WCS and frame
  imghelp_advise.npz     advise_wide_field: every key of every case;
                         rad_deg_arcsec strings; visibility_recentre
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.modules["pyfftw"] = None

from make_golden import dm, load_reference, save  # noqa: E402

import imghelp_case as C  # noqa: E402


class _Hertz:
    """``x * units.Hz``: a float that also answers ``.to(unit).value``."""

    __array_ufunc__ = None  # numpy scalars defer to __rmul__

    def __rmul__(self, x):
        return _Quantity(x)


class _Quantity(float):
    def to(self, unit):
        return self

    @property
    def value(self):
        return float(self)


class _Units:
    Hz = _Hertz()


def make_sum(helpers):
    out = {}
    for name in C.INVERT_CASES:
        image_list = C.invert_list(name)
        before = [None if e is None else (e[0]["pixels"].data.copy(), e[1].copy())
                  for e in image_list]
        im, sumwt = helpers["sum_invert_results"](image_list)
        for e, b in zip(image_list, before):  # the inputs are left alone
            assert e is None or (np.array_equal(e[0]["pixels"].data, b[0], equal_nan=True)
                                 and np.array_equal(e[1], b[1]))
        assert im.attrs["clean_beam"] == C.CLEAN_BEAM
        out[f"invert_{name}_pixels"] = im["pixels"].data
        out[f"invert_{name}_sumwt"] = sumwt
    assert not out["invert_zero_plane_pixels"][1, 0].any()
    assert np.signbit(out["invert_zero_plane_pixels"][1, 0]).sum() == 0
    pairs = C.invert_list("negative")
    assert all(a is b[0] for a, b in zip(helpers["remove_sumwt"](pairs), pairs))

    results = C.predict_list()
    summed = helpers["sum_predict_results"](results)
    assert summed is results[1]
    out["predict_vis"] = summed["vis"].data
    assert helpers["sum_predict_results"]([None, None]) is None
    save("imghelp_sum.npz", **out)


def make_threshold(helpers):
    out = {}
    for name, (images, threshold, fraction, moment0) in C.THRESHOLD_CASES.items():
        out[name] = np.array(helpers["threshold_list"](C.threshold_list_input(images), threshold,
                                                       fraction, use_moment0=moment0))
    save("imghelp_threshold.npz", **out)


def make_image(base):
    out = {}
    for name, (kind, kwargs) in C.IMAGE_CASES.items():
        im = base["create_image_from_visibility"](C.make_vis(kind), **C.image_kwargs(kwargs))
        for key, value in C.image_summary(im).items():
            out[f"{name}_{key}"] = value
    try:
        base["create_image_from_visibility"](C.make_vis(C.IMAGE_REFUSED[0]), **C.IMAGE_REFUSED[1])
        raise AssertionError("the refused case was accepted")
    except ValueError:
        pass
    save("imghelp_image.npz", **out)


def make_advise(base):
    out = {}
    for name, (kind, kwargs) in C.ADVISE_CASES.items():
        advice = base["advise_wide_field"](C.make_vis(kind), **kwargs)
        out[f"{name}_keys"] = np.array(list(advice))
        for key, value in advice.items():
            out[f"{name}_{key}"] = np.array(value)
    out["rad_deg_arcsec"] = np.array([base["rad_deg_arcsec"](x) for x in C.RAD_DEG_ARCSEC_INPUTS])
    uvw, dl, dm_ = C.recentre_input()
    out["recentre"] = base["visibility_recentre"](uvw, dl, dm_)
    save("imghelp_advise.npz", **out)


def main():
    base = load_reference(
        "imaging/base.py",
        ["create_image_from_visibility", "advise_wide_field", "rad_deg_arcsec",
         "visibility_recentre", "normalise_sumwt"],
        {"units": _Units, "PolarisationFrame": dm.PolarisationFrame,
         "create_image": dm.create_image})
    taylor = load_reference("image/taylor_terms.py", ["calculate_image_frequency_moments"])
    helpers = load_reference(
        "imaging/imaging_helpers.py",
        ["sum_invert_results", "remove_sumwt", "sum_predict_results", "threshold_list"],
        {"normalise_sumwt": base["normalise_sumwt"],
         "calculate_image_frequency_moments": taylor["calculate_image_frequency_moments"]})
    make_sum(helpers)
    make_threshold(helpers)
    make_image(base)
    make_advise(base)


if __name__ == "__main__":
    main()
