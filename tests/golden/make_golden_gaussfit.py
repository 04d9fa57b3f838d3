"""Writes tests/golden/gaussfit_windows.npz and gaussfit_image.npz from the
host restatement of fit_skycomponent (tests/gaussfit_restatement.py: numpy and
scipy.optimize.leastsq, the MINPACK solver the reference runs through astropy;
not a run of the reference, astropy being absent here).

Run from the repository root:  python tests/golden/make_golden_gaussfit.py

gaussfit_windows.npz, per case of gaussfit_restatement.WINDOW_CASES: the 15 x
15 window, its home (x0, y0), the yardstick's parameters at the reference's
stop ("default") and at xtol = ftol = 1e-14 ("tight"), the evaluations of both.
gaussfit_image.npz: the pixels of gaussfit_restatement.image_case, per
component whether it is fitted, both parameter sets, and the post-processed
fields from the tight parameters with force_point_sources True and False.

Both hold S [6]: per parameter the largest |default - tight| over every
committed fit (theta: over the fits with an axial ratio of at least 1.3).  The
tests ask the device's parameters to lie within 2 S of the tight ones.

Asserted here, so that no case needs excusing: every fit is "converged" in
the yardstick at both stops, and every tight centre is at least 0.05 pixel from
a half-integer in x and in y.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "ska-sdp-func-python_amd"))

import gaussfit_restatement as gr  # noqa: E402


def spread(default, tight):
    d = np.abs(np.asarray(default) - np.asarray(tight))
    d[gr.axial_ratio(tight) < gr.THETA_AXIAL_RATIO, 5] = 0.0
    return d.max(axis=0)


def check(name, default, tight):
    assert default["converged"] and tight["converged"], f"{name}: the yardstick did not converge"
    margin = gr.half_pixel_margin(tight["params"])
    assert margin >= gr.HALF_PIXEL_MARGIN, f"{name}: centre {margin:.3f} from a half-integer"
    assert np.all(np.round(default["params"][1:3]) == np.round(tight["params"][1:3]))


def windows():
    names = list(gr.WINDOW_CASES)
    z = np.stack([gr.case_window(n) for n in names])
    home = np.array([gr.WINDOW_HOMES[n] for n in names])
    default, tight, nfev, shuffled = [], [], [], []
    order = np.random.default_rng(5).permutation(gr.WINDOW ** 2)
    for k, n in enumerate(names):
        d = gr.fit_window(z[k], *home[k])
        t = gr.fit_window(z[k], *home[k], tight=True)
        check(n, d, t)
        s = gr.fit_window(z[k], *home[k], tight=True, order=order)
        default.append(d["params"])
        tight.append(t["params"])
        shuffled.append(np.abs(s["params"] - t["params"]))
        nfev.append((d["nfev"], t["nfev"]))
        print(f"{n:18s} nfev {d['nfev']:3d} / {t['nfev']:3d}  axial ratio "
              f"{gr.axial_ratio(t['params']):.2f}  |default - tight| "
              f"{np.abs(d['params'] - t['params']).max():.1e}")
    print("tight against itself with the pixels shuffled:", np.max(shuffled, axis=0))
    return dict(names=np.array(names), windows=z, home=home, default=np.array(default),
                tight=np.array(tight), nfev=np.array(nfev))


def image():
    im, comps = gr.image_case()
    out = dict(pixels=np.asarray(im["pixels"].data), fitted=[], default=[], tight=[], ra=[], dec=[],
               flux=[], beam=[])
    for k, sc in enumerate(comps):
        d = gr.fit_component(im, sc)
        t = gr.fit_component(im, sc, tight=True)
        g = gr.fit_component(im, sc, tight=True, force_point_sources=False)
        assert d["fitted"] == t["fitted"] == g["fitted"]
        if t["fitted"]:
            check(f"image component {k}", dict(params=d["fit"], converged=True),
                  dict(params=t["fit"], converged=True))
            assert t["shape"] == "Point" and g["shape"] == "Gaussian"
        out["fitted"].append(t["fitted"])
        nan6 = np.full(6, np.nan)
        out["default"].append(d["fit"] if d["fitted"] else nan6)
        out["tight"].append(t["fit"] if t["fitted"] else nan6)
        out["ra"].append(t["ra"])
        out["dec"].append(t["dec"])
        out["flux"].append(t["flux"])
        p = g["params"]
        out["beam"].append([p["bmaj"], p["bmin"], p["bpa"]] if g["fitted"] else [np.nan] * 3)
    return {k: np.array(v) for k, v in out.items()}


def image_converged():
    """The converged flags of the image's fits (fit_component does not return them)."""
    im, comps = gr.image_case()
    pixels = np.asarray(im["pixels"].data)
    from ska_sdp_func_python_amd import datamodels as dm
    for sc in comps:
        px, py = dm.skycoord_to_pixel(sc.direction, im.image_acc.wcs, origin=0)
        x0, y0 = gr.window_origin(np.round([px[0], py[0]]).astype(int))
        if gr.on_plane(x0, y0, *pixels.shape[2:]):
            for tight in (False, True):
                assert gr.fit_plane(pixels[0, 0], x0, y0, tight)["converged"]


def main():
    w = windows()
    image_converged()
    i = image()
    fitted = i["fitted"]
    assert list(fitted) == [True, True, False, False]
    S = np.maximum(spread(w["default"], w["tight"]), spread(i["default"][fitted], i["tight"][fitted]))
    print("S =", dict(zip(gr.NAMES, S)))
    np.savez(os.path.join(HERE, "gaussfit_windows.npz"), S=S, **w)
    np.savez(os.path.join(HERE, "gaussfit_image.npz"), S=S, **i)


if __name__ == "__main__":
    main()
