"""The imaging-weight cases of tests/weighting_cases.py, checked without a GPU:
each one must reach the branch of csrc/weighting.hip it is named for, so that
tests/test_gpu_weighting_paths.py cannot pass vacuously.  The strategy a case
takes is derived from weighting_cases.host_rules, the restated host rules."""

import numpy as np
import pytest

import weighting_cases as wc

ALL = sorted(wc.GEOMETRY)


@pytest.mark.parametrize("name", ALL)
def test_case_is_not_degenerate(name):
    c = wc.case(name)
    nsamp = c["nrow"] * c["nchan"] * c["npol"]
    assert 0 < c["ref_skip"] < nsamp / 2
    planes = c["ref_grid"].reshape(-1, c["ny"], c["nx"])
    assert c["npol"] * c["g_nchan"] == 1 or (planes.reshape(len(planes), -1).any(1).sum() > 1)
    if c["npol"] > 1:
        assert not np.array_equal(c["ref_grid"][:, 0], c["ref_grid"][:, 1])
    if c["g_nchan"] > 1:
        assert not np.array_equal(c["ref_grid"][0], c["ref_grid"][1])
    # dyadic: everything gridded is a multiple of 1/8 and the total is exact
    assert np.array_equal(c["ref_grid"] * 8, np.round(c["ref_grid"] * 8))
    assert np.array_equal(c["ref_grid"].sum((2, 3)), c["ref_sumwt"])
    if c["flags"] is not None:
        assert set(np.unique(c["flags"])) == {0, 1}


def test_dyadic_weights_differ_between_pols_and_channels():
    w = wc.dyadic_weights((50, 6, 4), 1)
    assert w.min() >= 0.125 and w.max() <= 2.0 and np.array_equal(w * 8, np.round(w * 8))
    assert len(np.unique(w)) == 16
    assert not np.array_equal(w[..., 0], w[..., 1]) and not np.array_equal(w[:, 0], w[:, 1])


def test_expected_strategy_of_each_case():
    """The branch each case is for, from the restated host rules."""
    r = {n: wc.host_rules(wc.case(n)) for n in ALL}
    assert r["rect_mirror"]["mirror"] and r["rect_mirror"]["win"] == 32
    assert wc.host_rules(wc.case("rect_mirror"), {"SDP_HIP_WEIGHT_NT": "256"})["win"] == 16
    assert wc.host_rules(wc.case("rect_mirror"), {"SDP_HIP_WEIGHT_WIN": "0"})["win"] == 0
    assert wc.host_rules(wc.case("rect_mirror"), {"SDP_HIP_WEIGHT_WIN": "8"})["win"] == 8
    assert not wc.host_rules(wc.case("rect_mirror"), {"SDP_HIP_WEIGHT_NOMIRROR": "1"})["mirror"]
    assert r["rect_mirror"]["win_u0"] != r["rect_mirror"]["win_v0"]
    assert r["frac_crpix"]["zero_val"] and not r["frac_crpix"]["mirror"] and r["frac_crpix"]["win"]
    assert not r["shifted"]["zero_val"] and not r["shifted"]["mirror"] and r["shifted"]["win"]
    assert r["tiny"]["win"] == 0 and r["tiny"]["mirror"]
    assert r["planes260"]["win"] == 0 and not r["planes260"]["lds_sum"]
    assert not r["nchan1030"]["lds_k"] and r["nchan1030"]["win"] == 64
    assert all(v["lds_k"] for k, v in r.items() if k != "nchan1030")
    assert all(v["lds_sum"] for k, v in r.items() if k != "planes260")
    for n in ("frac_crpix", "tiny", "ties_rect"):   # nchan 9, npol 1
        assert r[n]["odd_full_span"] and r[n]["tail_span"] == 1
    assert not r["rect_mirror"]["odd_full_span"]
    assert r["ties"]["mirror"] and r["ties"]["win"] == 64 and r["ties"]["nplanes"] == 4
    assert r["ties_rect"]["mirror"] and r["ties_rect"]["win"] == 128


@pytest.mark.parametrize("name", wc.CLIPPED_CASES)
def test_clipped_window_splits_the_weight(name):
    """The window touches a grid edge.  Both a sample's cell and its conjugate
    cell must be on the grid, so on an axis where the window is clipped every
    gridded cell is inside it: rect_offcentre, clipped on both axes, has the
    whole gridded weight in the window (what it adds is the window offsets and
    a mirror image that leaves the grid), and rect_edge, clipped in v only,
    splits it between the window and global atomics."""
    c = wc.case(name)
    r = wc.host_rules(c)
    w = r["win"]
    edges = [r["win_u0"] == 0, r["win_u0"] + w == c["nx"], r["win_v0"] == 0,
             r["win_v0"] + w == c["ny"]]
    assert w > 0 and any(edges)
    total = c["ref_grid"].sum()
    inside = c["ref_grid"][:, :, r["win_v0"]:r["win_v0"] + w, r["win_u0"]:r["win_u0"] + w].sum()
    assert inside >= 0.1 * total
    if name == "rect_offcentre":
        assert sum(edges) == 2 and inside == total
        # the mirror image of row 0 is off the grid (k_mirror_fold's range test)
        assert 2 * (c["wcs"][1][2] - 1) - 0 >= c["ny"]
    else:
        assert total - inside >= 0.1 * total


@pytest.mark.parametrize("name", wc.TIE_CASES)
def test_tie_case_reaches_the_tie_branch(name):
    c = wc.case(name)
    r = wc.host_rules(c)
    assert r["mirror"]
    pu, pv, puc, pvc, ok = wc.cells(c)
    tie = c["tie"]
    assert tie.sum() >= 100 and not (tie & ~ok).any()
    assert 0.15 < c["ntie_rows"] / c["nrow"] < 0.35
    inw = wc.in_window(r, pu, pv)
    assert (tie & inw).sum() >= 20
    assert (tie & ~inw).sum() >= 20
    # ties in u and in v, at the first, the last and the inner channels of a span
    cu2, cv2 = 2 * (c["wcs"][0][2] - 1), 2 * (c["wcs"][1][2] - 1)
    assert (tie & (pu + puc != cu2)).sum() >= 20 and (tie & (pv + pvc != cv2)).sum() >= 20
    pos = np.nonzero(tie)[1] % wc.K_CHAN
    assert (pos == 0).sum() >= 5 and (pos == wc.K_CHAN - 1).sum() >= 5
    assert ((pos > 0) & (pos < wc.K_CHAN - 1)).sum() >= 20
    # a tie in the middle of a run: the channel before it and the channel after
    # it, both in its span, are ordinary samples of one cell and image channel
    same = np.zeros_like(tie)
    other_ic = np.zeros_like(tie)
    v2i = c["v2i"]
    for ch in range(1, c["nchan"] - 1):
        if ch % wc.K_CHAN in (0, wc.K_CHAN - 1):
            continue
        a, b = ch - 1, ch + 1
        run = (ok[:, a] & ok[:, b] & ~tie[:, a] & ~tie[:, b] & (pu[:, a] == pu[:, b])
               & (pv[:, a] == pv[:, b]) & (puc[:, a] == puc[:, b]) & (pvc[:, a] == pvc[:, b])
               & (v2i[a] == v2i[b]))
        same[:, ch] = tie[:, ch] & run
        other_ic[:, ch] = same[:, ch] & (v2i[ch] != v2i[a])
    assert same.sum() >= 10
    if c["g_nchan"] > 1:
        # ... and the tie belongs to another image channel than the run
        assert other_ic.sum() >= 10
        assert np.any(np.diff(v2i) < 0)
