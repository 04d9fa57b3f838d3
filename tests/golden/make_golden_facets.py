"""Generate the facet fixtures tests/golden/facets_*.npz from the REFERENCE's
own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_facets.py

image_raster_iter with its tapers (image/iterators.py), image_scatter_facets
and image_gather_facets (image/gather_scatter.py) and tukey_filter
(util/array_functions.py) are AST-extracted and executed with numpy on the
datamodels shim, as make_golden.py does.  Only inputs, settings and outputs
are stored -- no reference source text.  The inputs are rebuilt by
tests/facets_case.py, which the tests share.

  facets_<case>.npz   for each case of facets_case.CASES: the image, the
                      gathered image of the scaled facets, the return_flat
                      image, the 1-D tapers, and the origin (y, x) and crpix
                      of every sub-image
  facets_refused.npz  the rasters (ny, nx, facets, overlap) that the
                      reference refuses with ValueError
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_reference, save  # noqa: E402

import facets_case as C  # noqa: E402


def reference():
    arr = load_reference("util/array_functions.py", ["tukey_filter"])
    it = load_reference("image/iterators.py",
                        ["_taper_linear", "_taper_quadratic", "_taper_tukey", "_taper_flat",
                         "_validate_data", "image_raster_iter"],
                        {"tukey_filter": arr["tukey_filter"]})
    gs = load_reference("image/gather_scatter.py", ["image_scatter_facets", "image_gather_facets"],
                        {"List": list, "image_raster_iter": it["image_raster_iter"]})
    return it, gs


def make_case(name, it, gs):
    ny, nx, facets, overlap, taper, dtype = C.CASES[name]
    pixels = C.case_pixels(name)
    im = C.make_image(pixels.copy())
    subs = gs["image_scatter_facets"](im, facets=facets, overlap=overlap, taper=taper)
    assert len(subs) == facets * facets
    base = im["pixels"].data
    dy, dx = subs[0]["pixels"].data.shape[2:]
    origins, crpix = [], []
    for sub in subs:
        view = sub["pixels"].data
        assert np.shares_memory(view, base) and view.shape == (C.NCHAN, 2, dy, dx)
        offset = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) \
            // base.itemsize
        origins.append(divmod(offset, nx))
        crpix.append(sub.image_acc.wcs.wcs.crpix.copy())
    scaled = C.facet_images(subs)
    gathered = gs["image_gather_facets"](scaled, im, facets=facets, overlap=overlap, taper=taper)
    flat = gs["image_gather_facets"](scaled, im, facets=facets, overlap=overlap, taper=taper,
                                     return_flat=True)
    assert np.array_equal(im["pixels"].data, pixels)  # the template is not written
    assert gathered["pixels"].data.dtype == pixels.dtype and flat["pixels"].data.dtype == pixels.dtype
    fn = {"linear": it["_taper_linear"], "quadratic": it["_taper_quadratic"],
          "tukey": it["_taper_tukey"]}.get(taper)
    taper_y = np.asarray(fn(dy, overlap) if fn and overlap > 0 else it["_taper_flat"](dy), float)
    taper_x = np.asarray(fn(dx, overlap) if fn and overlap > 0 else it["_taper_flat"](dx), float)
    save(f"facets_{name}.npz", pixels=pixels, gathered=gathered["pixels"].data,
         flat=flat["pixels"].data, taper_y=taper_y, taper_x=taper_x,
         origins=np.array(origins), crpix=np.array(crpix),
         settings=np.array([ny, nx, facets, overlap]), taper=np.array(str(taper)))


def make_refused(gs):
    for ny, nx, facets, overlap in C.REFUSED:
        im = C.make_image(C.image_pixels(ny, nx))
        try:
            gs["image_scatter_facets"](im, facets=facets, overlap=overlap)
        except ValueError as err:
            print("refused", (ny, nx, facets, overlap), err)
        else:
            raise AssertionError((ny, nx, facets, overlap))
    save("facets_refused.npz", rasters=np.array(C.REFUSED))


def main():
    it, gs = reference()
    for name in C.CASES:
        make_case(name, it, gs)
    make_refused(gs)


if __name__ == "__main__":
    main()
