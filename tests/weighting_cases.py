"""Imaging-weight cases shared by tests/test_weighting_cases_cpu.py (which
checks that each case reaches the branch it is named for) and
tests/test_gpu_weighting_paths.py (which runs them through the HIP gridder).

Plain numpy; the reference is oracle/weighting_oracle.py.  Weights are dyadic
(k/8), so every gridded sum is exact in any order and grid, sumwt and uniform
weights compare bit for bit while polarisations and channels still differ.

``host_rules`` restates how csrc/weighting.hip's make_geom / choose_window
pick the accumulation strategy, so a test can say which branch a case takes
without asking the kernel.
"""

import functools
import math

import numpy as np

import weighting_oracle as wo

K_CHAN = 8          # channels per thread span
MAX_LDS_SUM = 256   # planes whose sumwt lives in LDS
MAX_LDS_K = 1024    # channels whose freq / c lives in LDS

NONMONO = [0, 1, 0, 1, 1, 0, 1, 0]

# name: ny, nx, crpix (u, v), crval in cells (u, v), nchan, npol, g_nchan, flags, rows, map
GEOMETRY = {
    "rect_mirror":    (96, 160, (81, 49), (0, 0), 16, 4, 2, np.int64, 6000, "mono"),
    "rect_offcentre": (96, 160, (20, 70), (0, 0), 12, 2, 1, np.int8, 6000, "mono"),
    "rect_edge":      (96, 160, (70, 12), (0, 0), 16, 4, 2, np.int32, 6000, "mono"),
    "frac_crpix":     (128, 96, (48.5, 64.5), (0, 0), 9, 1, 2, None, 6000, "mono"),
    "shifted":        (96, 160, (81, 49), (0.37, -0.21), 16, 4, 2, np.int32, 6000, "mono"),
    "tiny":           (6, 10, (6, 4), (0, 0), 9, 1, 2, np.int8, 2000, "mono"),
    "nchan1030":      (96, 160, (81, 49), (0, 0), 1030, 1, 2, np.int64, 64, "mono"),
    "planes260":      (32, 24, (13, 17), (0, 0), 65, 4, 65, np.int32, 2000, "mono"),
    "ties":           (1024, 1024, (513, 513), (0, 0), 16, 2, 2, np.int64, 4800, "nonmono"),
    "ties_rect":      (192, 320, (161, 97), (0, 0), 9, 1, 1, None, 3000, "mono"),
}
TIE_CASES = ("ties", "ties_rect")
CLIPPED_CASES = ("rect_offcentre", "rect_edge")


def dyadic_weights(shape, seed):
    """k/8 with k in 1..16: any sum of fewer than 2^46 of them is exact."""
    return np.random.default_rng(seed).integers(1, 17, shape).astype(float) / 8.0


def _mid_uvw(nrows, seed):
    """``nrows`` baselines of one SKA-MID snapshot, drawn without replacement."""
    from ska_sdp_func_python_amd import simulation
    fn, n_def, lat, dec = simulation.CONFIGS["MID"]
    uvw, _ = simulation.observe(fn(n_def, seed=1), math.radians(lat), math.radians(dec),
                                np.array([0.1]))
    uvw = uvw.reshape(-1, 3)
    pick = np.random.default_rng(seed).choice(uvw.shape[0], nrows, replace=False)
    return np.ascontiguousarray(uvw[np.sort(pick)])


def _tie_freq(nchan):
    """Groups of four channels 2% apart; inside a group the frequencies differ
    by parts in 10^9 in the order 0, 2, 1, 3, so that the channels on either
    side of the second and third of a group fall in one cell."""
    c = np.arange(nchan)
    return 1.0e9 * (1.0 + 0.02 * (c // 4)) * (1.0 + 1e-9 * np.array([0, 2, 1, 3])[c % 4])


def tie_mask(uvw, freq, wcs, ny, nx):
    """[nrow, nchan] bool: in-grid samples whose conjugate cell is not the
    mirror image of their cell about the cell of u = v = 0."""
    cu2, cv2 = 2 * (wcs[0][2] - 1), 2 * (wcs[1][2] - 1)
    out = np.zeros((uvw.shape[0], len(freq)), dtype=bool)
    for ch in range(len(freq)):
        pu, pv, puc, pvc = wo.mapping(uvw, freq, ch, wcs)
        ok = wo._ingrid(pu, pv, puc, pvc, ny, nx)
        out[:, ch] = ok & ((pu + puc != cu2) | (pv + pvc != cv2))
    return out


def tie_rows(freq, wcs, ny, nx, m_range, seed, steps=48, per_offset=3):
    """Rows with one sample at an exact rounding tie.  For each half-cell
    offset m + 0.5 (m in ``m_range``) and a channel c that cycles through the
    band, u0 = (m + 0.5) |cdelt| / (freq[c] / C) and its ``steps`` nextafter
    neighbours on either side are mapped; up to ``per_offset`` of those whose
    cell and conjugate cell do not add up to twice the centre are kept, with an
    ordinary v.  The same again with u and v exchanged.  (Six neighbours reach
    ties from |m| of about 40; 48 reach them from |m| of about 8, inside a 64^2
    window.)  Returns (uvw [n, 3], mask [n, nchan])."""
    rng = np.random.default_rng(seed)
    nchan = len(freq)
    rows = []
    idx = 0
    for axis in (0, 1):
        other = 1 - axis
        half_other = min(wcs[other][2] - 1, (nx, ny)[other] - wcs[other][2])
        for m in range(*m_range[axis]):
            c = idx % nchan
            k = freq[c] / wo.C_M_S
            x0 = (m + 0.5) * abs(wcs[axis][1]) / k
            cand = [x0]
            lo = hi = x0
            for _ in range(steps):
                lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
                cand += [lo, hi]
            # the other coordinate: well inside a cell, near the centre for
            # every other row and anywhere on the grid for the rest
            span = 24 if idx % 2 == 0 else int(0.9 * half_other)
            j = int(rng.integers(-span, span + 1))
            y0 = (j + 0.3) * abs(wcs[other][1]) / k
            uvw = np.zeros((len(cand), 3))
            uvw[:, axis] = cand
            uvw[:, other] = y0
            pu, pv, puc, pvc = wo.mapping(uvw, freq, c, wcs)
            ok = wo._ingrid(pu, pv, puc, pvc, ny, nx)
            tie = ok & ((pu + puc != 2 * (wcs[0][2] - 1)) | (pv + pvc != 2 * (wcs[1][2] - 1)))
            rows += [uvw[i] for i in np.nonzero(tie)[0][:per_offset]]
            idx += 1
    uvw = np.array(rows)
    return uvw, tie_mask(uvw, freq, wcs, ny, nx)


def host_rules(case, env=None):
    """make_geom + choose_window of csrc/weighting.hip, restated: which
    strategy the gridder takes for ``case`` under the SDP_HIP_WEIGHT_*
    variables in ``env``."""
    env = env or {}
    (uval, udel, upix), (vval, vdel, vpix) = case["wcs"]
    ny, nx = case["ny"], case["nx"]
    nplanes = case["g_nchan"] * case["npol"]
    nt = 256 if int(env.get("SDP_HIP_WEIGHT_NT", 1024)) == 256 else 1024
    zero_val = uval == 0.0 and vval == 0.0
    mirror = (zero_val and upix == math.floor(upix) and vpix == math.floor(vpix)
              and "SDP_HIP_WEIGHT_NOMIRROR" not in env)
    win = int(env.get("SDP_HIP_WEIGHT_WIN", 128))
    budget = 131072 if nt == 1024 else 32768
    while win >= 8 and (nplanes * win * win * 8 > budget or win > nx or win > ny):
        win //= 2
    u0 = v0 = 0
    if win < 8:
        win = 0
    else:
        # round-half-even like nearbyint
        u0 = int(np.rint((0.0 - uval) / udel + upix - 1.0)) - win // 2
        v0 = int(np.rint((0.0 - vval) / vdel + vpix - 1.0)) - win // 2
        u0 = max(0, min(u0, nx - win))
        v0 = max(0, min(v0, ny - win))
    nchan, npol = case["nchan"], case["npol"]
    nspan = -(-nchan // K_CHAN)
    # a full span whose first element is odd takes the element-wise load
    odd_full = any((r * nchan * npol + s * K_CHAN * npol) % 2 == 1
                   for r in range(2) for s in range(nspan)
                   if min(K_CHAN, nchan - s * K_CHAN) == K_CHAN)
    return dict(win=win, win_u0=u0, win_v0=v0, mirror=bool(mirror), zero_val=bool(zero_val),
                nplanes=nplanes, nt=nt, lds_sum=nplanes <= MAX_LDS_SUM, lds_k=nchan <= MAX_LDS_K,
                odd_full_span=odd_full, tail_span=nchan % K_CHAN)


def in_window(rules, pu, pv):
    w = rules["win"]
    return ((w > 0) & (pu >= rules["win_u0"]) & (pu < rules["win_u0"] + w)
            & (pv >= rules["win_v0"]) & (pv < rules["win_v0"] + w))


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of case ``name`` and the oracle's grid, sumwt and skip count
    for them (computed once and shared; treat every array as read-only)."""
    ny, nx, crpix, crval_cells, nchan, npol, g_nchan, fdtype, nrows, vmap = GEOMETRY[name]
    seed = sorted(GEOMETRY).index(name) + 11
    rng = np.random.default_rng(seed)
    tie = name in TIE_CASES
    freq = _tie_freq(nchan) if tie else np.linspace(0.95e9, 1.76e9, nchan)
    uvw = _mid_uvw(nrows, seed)
    # cell size per axis: 5% of the |u| (|v|) at the top of the band reach
    # past the symmetric part of the grid, so a few percent are skipped
    kmax = freq.max() / wo.C_M_S
    half = [min(crpix[0] - 1, nx - crpix[0]), min(crpix[1] - 1, ny - crpix[1])]
    du = np.quantile(np.abs(uvw[:, 0]), 0.95) * kmax / half[0]
    dv = np.quantile(np.abs(uvw[:, 1]), 0.95) * kmax / half[1]
    wcs = ((crval_cells[0] * du, -du, crpix[0]), (crval_cells[1] * dv, dv, crpix[1]))
    ntie_rows = 0
    if tie:
        m_range = [(-min(200, int(half[0]) - 4), min(200, int(half[0]) - 4)),
                   (-min(200, int(half[1]) - 4), min(200, int(half[1]) - 4))]
        t_uvw, _ = tie_rows(freq, wcs, ny, nx, m_range, seed)
        ntie_rows = t_uvw.shape[0]
        uvw = np.concatenate([t_uvw, uvw[:max(3 * ntie_rows, 2000 - ntie_rows)]])
        uvw = np.ascontiguousarray(uvw[rng.permutation(uvw.shape[0])])
    nrow = uvw.shape[0]
    shape = (nrow, nchan, npol)
    wt = dyadic_weights(shape, seed + 100)
    flags = None if fdtype is None else (rng.uniform(size=shape) < 0.05).astype(fdtype)
    if vmap == "nonmono":
        v2i = np.array((NONMONO * (nchan // 8 + 1))[:nchan])
    else:
        v2i = (np.arange(nchan) * g_nchan) // nchan
    fwt = wt if flags is None else wt * (1 - flags)
    grid, sumwt, skip = wo.grid_weights(uvw, freq, fwt, v2i, wcs, g_nchan, ny, nx)
    assert skip > 0, name
    imw = dyadic_weights(shape, seed + 200) * 3.0
    out = dict(name=name, uvw=uvw, freq=freq, wt=wt, flags=flags, fwt=fwt, imw=imw,
               fimw=imw if flags is None else imw * (1 - flags), v2i=v2i, wcs=wcs,
               g_nchan=g_nchan, ny=ny, nx=nx, nchan=nchan, npol=npol, nrow=nrow,
               ref_grid=grid, ref_sumwt=sumwt, ref_skip=skip, ntie_rows=ntie_rows)
    if tie:
        out["tie"] = tie_mask(uvw, freq, wcs, ny, nx)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def cells(c):
    """(pu, pv, puc, pvc, ok) [nrow, nchan] of every sample of case dict ``c``."""
    p = np.zeros((4, c["nrow"], c["nchan"]), dtype=np.int64)
    ok = np.zeros(p.shape[1:], dtype=bool)
    for ch in range(c["nchan"]):
        m = wo.mapping(c["uvw"], c["freq"], ch, c["wcs"])
        p[:, :, ch] = m
        ok[:, ch] = wo._ingrid(*m, c["ny"], c["nx"])
    return p[0], p[1], p[2], p[3], ok
