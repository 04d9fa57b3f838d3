"""Host restatement of find_skycomponents (reference
src/ska_sdp_func_python/sky_component/operations.py:256-363) from numpy and
scipy.ndimage.label, the stand-ins that put it in place of the two kernel
wrappers (kernels.segment_image, kernels.segment_peaks), and the builders of
the test cases.  Used by tests/test_findcomp_cpu.py and
tests/test_gpu_findcomp.py.

This is the yardstick of those tests, and it is NOT a run of the reference:
neither astropy nor photutils is available where this project is built.  It
restates the five steps of the reference function:

1. mean plane: numpy.sum(pixels, axis=0)[0] / float(nchan) (:287-289), in the
   pixels' type;
2. smoothing: astropy 5.2.2 convolve with its defaults of a normalised
   Gaussian2DKernel of int(1.5 fwhm) pixels a side, made odd (:278-290):
   pixels off the image count as 0, the sum is divided by the kernel's;
3. segmentation: photutils 1.8.0 detect_sources (:291-293): smoothed >
   threshold, scipy.ndimage.label with the 3 x 3 structure of ones, segments
   of fewer than npixels pixels dropped, the rest renumbered in their order;
4. peaks: SourceCatalog's max_value and maxval_index per segment and channel
   of the unsmoothed Stokes-I plane (:299-315), the first pixel on ties;
5. the component (:319-361).

Step 3 calls scipy.ndimage.label, the very function photutils calls.  Steps 2
and 4 rest on the documented behaviour of astropy 5.2.2 and photutils 1.8.0
(the versions of the reference's poetry.lock:47-48 and :723-724), not on
running them.
"""

import contextlib

import numpy as np
from scipy import ndimage

TILE = 32  # the labelling kernel's tile (SDP_HIP_SEGMENT_TILE); the cases straddle it
# at least three tiles each way with a ragged last one; one row; one column;
# whole tiles
SHAPES = [(75, 150), (1, 97), (97, 1), (64, 96)]


# ---- the five steps ------------------------------------------------------------
def kernel_size(fwhm):
    size = int(1.5 * fwhm)
    return size + 1 if size % 2 == 0 else size


def kernel_of(fwhm):
    """The normalised Gaussian on kernel_size(fwhm) pixels a side."""
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    size = kernel_size(fwhm)
    if size == 1:
        return np.ones((1, 1))
    off = np.arange(size) - size // 2
    g = np.exp(-(off[:, None] ** 2 + off[None, :] ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def mean_plane(planes):
    """Step 1 of planes [nchan, ny, nx] (Stokes I of every channel)."""
    return np.sum(planes, axis=0) / float(planes.shape[0])


def smooth(mean, kernel):
    """Step 2: the window sum, rows then columns, over the kernel's sum."""
    mean = np.asarray(mean, dtype=np.float64)
    ny, nx = mean.shape
    K = kernel.shape[0]
    h = K // 2
    padded = np.zeros((ny + 2 * h, nx + 2 * h))
    padded[h:h + ny, h:h + nx] = mean
    acc = np.zeros((ny, nx))
    for dy in range(K):
        for dx in range(K):
            acc = acc + padded[dy:dy + ny, dx:dx + nx] * kernel[dy, dx]
    return acc / float(kernel.sum())


def label_mask(mask, npixels):
    """Step 3 of a boolean mask: (segment map int32, number of segments)."""
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    keep = sizes >= npixels
    keep[0] = False
    newid = np.where(keep, np.cumsum(keep), 0)
    return newid[lab].astype(np.int32), int(keep.sum())


def smoothed(planes, kernel=None):
    return smooth(mean_plane(np.asarray(planes)), np.ones((1, 1)) if kernel is None else kernel)


def segment(planes, threshold, npixels, kernel=None):
    """Steps 1-3 of planes [nchan, ny, nx]."""
    return label_mask(smoothed(planes, kernel) > threshold, npixels)


def peaks(planes, labels, nlabels):
    """Step 4: (values [nchan, nlabels] float64, flat indices [nchan, nlabels])."""
    planes = np.asarray(planes)
    nchan = planes.shape[0]
    values = np.zeros((nchan, nlabels))
    indices = np.zeros((nchan, nlabels), dtype=np.int64)
    for seg in range(nlabels):
        where = np.flatnonzero(labels.ravel() == seg + 1)
        for chan in range(nchan):
            v = planes[chan].ravel()[where]
            first = int(np.argmax(v))  # the first maximum
            values[chan, seg] = v[first]
            indices[chan, seg] = where[first]
    return values, indices


def find(im, fwhm=1.0, threshold=1.0, npixels=5):
    """Steps 1-5 of an Image with numpy pixels: a list of dicts (ra, dec, x, y,
    flux [nchan, npol], name) in segment order."""
    from ska_sdp_func_python_amd import datamodels as dm
    pixels = np.asarray(im["pixels"].data)
    nx = pixels.shape[3]
    labels, n = segment(pixels[:, 0], threshold, npixels, kernel_of(fwhm))
    if n == 0:
        raise ValueError("find_skycomponents: Failed to find any components")
    values, indices = peaks(pixels[:, 0], labels, n)
    wcs = im.image_acc.wcs
    out = []
    for seg in range(n):
        flux = values[:, seg]
        xs = (indices[:, seg] % nx).astype(float)
        ys = (indices[:, seg] // nx).astype(float)
        sc = [dm.pixel_to_skycoord(x, y, wcs, 0) for x, y in zip(xs, ys)]
        ras = np.array([c.ra.rad for c in sc])
        decs = np.array([c.dec.rad for c in sc])
        aflux = np.abs(flux)
        total = np.sum(aflux)
        x = np.sum(aflux * xs) / total
        y = np.sum(aflux * ys) / total
        out.append(dict(ra=np.sum(aflux * ras) / total, dec=np.sum(aflux * decs) / total, x=x, y=y,
                        flux=pixels[:, :, np.round(y).astype("int"), np.round(x).astype("int")],
                        name=f"Segment {seg}"))
    return out


# ---- stand-ins for the kernel wrappers (CPU tensors in place of device ones) --
def fake_segment_image(planes, threshold, npixels, kernel=None):
    import torch
    p = planes.numpy()
    if not np.isfinite(mean_plane(p)).all():
        raise ValueError("segment_image: the image has a pixel that is not finite")
    labels, n = segment(p, threshold, npixels, kernel)
    return torch.as_tensor(labels), n


def fake_segment_peaks(planes, labels, nlabels):
    import torch
    values, indices = peaks(planes.numpy(), labels.numpy(), nlabels)
    return torch.as_tensor(values), torch.as_tensor(indices)


@contextlib.contextmanager
def host_kernels():
    """Inside, find_skycomponents and segment_image run their own host code
    with the two kernel wrappers replaced by the restatement, on CPU tensors."""
    import torch
    from ska_sdp_func_python_amd import _device, kernels
    swaps = [(_device, "device", lambda: torch.device("cpu")),
             (kernels, "segment_image", fake_segment_image),
             (kernels, "segment_peaks", fake_segment_peaks)]
    saved = [getattr(mod, name) for mod, name, _ in swaps]
    try:
        for mod, name, new in swaps:
            setattr(mod, name, new)
        yield
    finally:
        for (mod, name, _), old in zip(swaps, saved):
            setattr(mod, name, old)


# ---- case builders ---------------------------------------------------------------
def random_mask(ny, nx, fill, seed):
    return np.random.default_rng(seed).random((ny, nx)) < fill


def spiral(ny, nx, pitch=2):
    """A one-pixel-wide rectangular spiral from the corner inwards whose arms
    lie ``pitch`` pixels apart."""
    m = np.zeros((ny, nx), dtype=bool)
    y = x = 0
    m[0, 0] = True
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    d = 0

    def free(y, x, dy, dx):
        ty, tx = y + dy, x + dx
        if not (0 <= ty < ny and 0 <= tx < nx) or m[ty, tx]:
            return False
        for k in range(1, pitch):
            ay, ax = ty + k * dy, tx + k * dx
            if 0 <= ay < ny and 0 <= ax < nx and m[ay, ax]:
                return False
        return True

    while True:
        if free(y, x, *dirs[d]):
            y, x = y + dirs[d][0], x + dirs[d][1]
            m[y, x] = True
            continue
        d = (d + 1) % 4
        if not free(y, x, *dirs[d]):
            return m


def two_spirals(ny, nx):
    """A spiral of pitch 4 and, in the corridor between its arms, the largest
    region that keeps a pixel's distance from it: they never touch, not even
    diagonally."""
    a = spiral(ny, nx, 4)
    rest = ~ndimage.binary_dilation(a, structure=np.ones((3, 3), dtype=bool))
    lab, n = ndimage.label(rest, structure=np.ones((3, 3), dtype=int))
    if n == 0:
        return a
    sizes = np.bincount(lab.ravel())[1:]
    return a | (lab == 1 + int(np.argmax(sizes)))


def staircase(ny, nx, anti=False):
    """Pixels joined only by their corners: the diagonal, which passes through
    every tile corner, or the anti-diagonal x + y = 2 TILE - 1."""
    m = np.zeros((ny, nx), dtype=bool)
    if anti:
        for y in range(ny):
            x = 2 * TILE - 1 - y
            if 0 <= x < nx:
                m[y, x] = True
    else:
        n = min(ny, nx)
        m[np.arange(n), np.arange(n)] = True
    return m


def checkerboard(ny, nx):
    y, x = np.indices((ny, nx))
    return (x + y) % 2 == 0


def comb(ny, nx, side):
    """Teeth two pixels apart that only the last row ("down"), the first row
    ("up"), the last column ("right") or the first column ("left") joins: for
    all but "up" and "left" the first pixel of the segment lies in another
    tile than the pixels that join its parts."""
    m = np.zeros((ny, nx), dtype=bool)
    if side in ("down", "up"):
        m[:, ::2] = True
        m[-1 if side == "down" else 0, :] = True
    else:
        m[::2, :] = True
        m[:, -1 if side == "right" else 0] = True
    return m


def nested_u(ny, nx):
    """U shapes inside one another, open to the top, two pixels apart: every U
    is a segment of its own whose two arms meet only at its bottom."""
    m = np.zeros((ny, nx), dtype=bool)
    for k in range(0, min(ny, nx // 2), 2):
        if nx - 1 - k <= k:
            break
        m[0:ny - k, k] = True
        m[0:ny - k, nx - 1 - k] = True
        m[ny - 1 - k, k:nx - k] = True
    return m


def bars(ny, nx, npixels):
    """Horizontal bars of exactly npixels and npixels - 1 pixels in turn, two
    pixels apart, some across the tile borders; returns (mask, bars kept)."""
    m = np.zeros((ny, nx), dtype=bool)
    kept = 0
    turn = 0
    for y in range(0, ny, 2):
        x = (3 * y) % 7
        while True:
            n = npixels - (turn % 2)
            if x + n > nx:
                break
            m[y, x:x + n] = True
            kept += n >= npixels
            turn += 1
            x += n + 2
    return m, kept


def mask_cases(ny, nx):
    """(name, mask) of every shape case on an ny x nx image."""
    cases = [(f"random{int(100 * fill)}", random_mask(ny, nx, fill, 100 + i))
             for i, fill in enumerate((0.30, 0.45, 0.60))]
    cases += [("spiral", spiral(ny, nx)), ("two_spirals", two_spirals(ny, nx)),
              ("staircase", staircase(ny, nx)), ("staircase_anti", staircase(ny, nx, True)),
              ("checkerboard", checkerboard(ny, nx)), ("nested_u", nested_u(ny, nx)),
              ("full", np.ones((ny, nx), dtype=bool))]
    cases += [(f"comb_{side}", comb(ny, nx, side)) for side in ("down", "up", "right", "left")]
    return cases


def planes_of(mask, dtype=np.float64):
    """One channel that is 1 on the mask and 0 off it (threshold 0.5)."""
    return mask.astype(dtype)[None]


def blobs_image(ny, nx, nchan, seed, sigma=1.7, nblobs=9, noise=0.05):
    """Seeded noise plus Gaussian blobs, some centred on the image's border;
    [nchan, ny, nx] float64, every channel with its own noise and amplitudes."""
    rng = np.random.default_rng(seed)
    y, x = np.indices((ny, nx))
    cy = rng.uniform(0, ny - 1, nblobs)
    cx = rng.uniform(0, nx - 1, nblobs)
    cy[:2] = (0, ny - 1)
    cx[2:4] = (0, nx - 1)
    planes = noise * rng.standard_normal((nchan, ny, nx))
    for k in range(nblobs):
        g = np.exp(-((y - cy[k]) ** 2 + (x - cx[k]) ** 2) / (2 * sigma ** 2))
        planes += rng.uniform(0.5, 2.0, nchan)[:, None, None] * g[None]
    return planes


def margin_ok(planes, fwhm, threshold):
    """The condition under which a device smoothing that rounds its window sum
    in another order gives the same mask: no smoothed value within 1e-9 of the
    largest magnitude of the threshold."""
    s = smoothed(planes, kernel_of(fwhm))
    return bool(np.min(np.abs(s - threshold)) > 1e-9 * np.max(np.abs(s)))
