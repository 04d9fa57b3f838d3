"""Generate the visibility-operation golden fixtures tests/golden/visops_*.npz
from the REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_visops.py

The reference's visibility/operations.py functions (integrate_visibility_by_channel
:192-235, average_visibility_by_channel :238-306, convert_visibility_to_stokes
:309-333, convert_visibility_to_stokesI :336-420,
convert_visibility_stokesI_to_polframe :423-471, remove_continuum_visibility
:108-142) are AST-extracted and executed with numpy on the datamodels shim, as
make_golden.py does.  Only inputs and outputs are stored -- no reference
source text.

ska-sdp-datamodels' convert_linear_to_stokes / convert_circular_to_stokes are
the shim's convert_pol_frame; its convert_linear_to_stokesI /
convert_circular_to_stokesI, which the shim does not have, are passed in as
the half-sum of the two parallel hands (what the Stokes matrices give for I).

Base case: simulation.make_visibility("LOW", nants=6, ntimes=2, nchan=8), random
complex vis, weights and imaging weights uniform(0.5, 2), about 15% of the
samples flagged, (time 0, baseline 3, pol 0) flagged on all channels and
(time 1, baseline 5, last pol) on all but channel 2.

Fixtures:
  visops_integrate_{linear,stokesI}.npz
  visops_average_linear.npz        channel_average 1, 2, 4, 8 (keys *_G<n>, the
                                   list stacked along the channel axis)
  visops_to_stokes_{linear,circular}.npz
  visops_to_stokesI_{linear,linearnp,circular,circularnp}.npz
  visops_polframe_linear.npz       stokesI -> linear
  visops_continuum_linear.npz      degree 0, 1, 2 without a mask, degree 1 with
      a mask (True on channels 3, 4, 5).  The reference raises LinAlgError on
      a spectrum without weight, so here the fully flagged spectrum keeps
      channels 1 and 6 (n_live = 2): it is rank deficient at degree 2; the
      spectrum flagged on all but one channel (n_live = 1) is rank deficient
      at degrees 1 and 2.  Every other spectrum has n_live > 2 (asserted).
"""

import os
import sys
from typing import List

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import dm, load_reference, save, simulation  # noqa: E402

NAMES = ["integrate_visibility_by_channel", "average_visibility_by_channel",
         "convert_visibility_to_stokes", "convert_visibility_to_stokesI",
         "convert_visibility_stokesI_to_polframe", "remove_continuum_visibility"]
MASK_CHANNELS = (3, 4, 5)


def _half_sum(v):
    return 0.5 * (v[..., 0] + v[..., -1])[..., np.newaxis]


def _reference():
    PF = dm.PolarisationFrame

    def conv(frame):
        return lambda v, polaxis: dm.convert_pol_frame(v, PF(frame), PF("stokesIQUV"), polaxis)

    return load_reference("visibility/operations.py", NAMES,
                          {"PolarisationFrame": PF, "List": List,
                           "convert_linear_to_stokes": conv("linear"),
                           "convert_circular_to_stokes": conv("circular"),
                           "convert_linear_to_stokesI": _half_sum,
                           "convert_circular_to_stokesI": _half_sum})


def base_case(frame, seed, continuum=False):
    rng = np.random.default_rng(seed)
    vis = simulation.make_visibility("LOW", nants=6, ntimes=2, nchan=8, f_lo=1.0e8, f_hi=1.1e8,
                                     polarisation_frame=frame)
    shape = vis.vis.shape
    npol = shape[3]
    vis["vis"].data = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    vis["weight"].data = rng.uniform(0.5, 2.0, shape)
    vis["imaging_weight"].data = rng.uniform(0.5, 2.0, shape)
    flags = (rng.uniform(size=shape) < 0.15).astype(int)
    flags[0, 3, :, 0] = 1
    flags[1, 5, :, npol - 1] = 1
    flags[1, 5, 2, npol - 1] = 0
    if continuum:
        flags[0, 3, 1, 0] = 0
        flags[0, 3, 6, 0] = 0
    vis["flags"].data = flags
    return vis


def inputs(vis, frame):
    return dict(vis=vis["vis"].data.copy(), weight=vis["weight"].data.copy(),
                imaging_weight=vis["imaging_weight"].data.copy(), flags=vis["flags"].data.copy(),
                frequency=np.asarray(vis.frequency.data),
                channel_bandwidth=np.asarray(vis.channel_bandwidth.data),
                time=np.asarray(vis.time.data),
                integration_time=np.asarray(vis.integration_time.data),
                uvw=np.asarray(vis.uvw.data), baselines=np.asarray(vis.baselines.data),
                frame=np.array(frame))


def outputs(v, tag):
    return {f"out_vis{tag}": np.asarray(v["vis"].data),
            f"out_weight{tag}": np.asarray(v["weight"].data),
            f"out_imaging_weight{tag}": np.asarray(v["imaging_weight"].data),
            f"out_flags{tag}": np.asarray(v["flags"].data).astype(np.int64),
            f"out_frequency{tag}": np.asarray(v.frequency.data),
            f"out_channel_bandwidth{tag}": np.asarray(v.channel_bandwidth.data),
            f"out_frame{tag}": np.array(v.visibility_acc.polarisation_frame.type)}


def main():
    ns = _reference()
    for i, frame in enumerate(("linear", "stokesI")):
        vis = base_case(frame, 61 + i)
        inp = inputs(vis, frame)
        save(f"visops_integrate_{frame}.npz", **inp,
             **outputs(ns["integrate_visibility_by_channel"](vis), ""))

    vis = base_case("linear", 63)
    out = inputs(vis, "linear")
    for G in (1, 2, 4, 8):
        lst = ns["average_visibility_by_channel"](vis, G)
        assert len(lst) == 8 // G
        for k in ("vis", "weight", "imaging_weight", "flags"):
            out[f"out_{k}_G{G}"] = np.concatenate([np.asarray(v[k].data) for v in lst], axis=2)
        out[f"out_frequency_G{G}"] = np.concatenate([np.asarray(v.frequency.data) for v in lst])
        out[f"out_channel_bandwidth_G{G}"] = np.concatenate(
            [np.asarray(v.channel_bandwidth.data) for v in lst])
    save("visops_average_linear.npz", **out)

    for i, frame in enumerate(("linear", "circular")):
        vis = base_case(frame, 64 + i)
        inp = inputs(vis, frame)
        res = ns["convert_visibility_to_stokes"](vis)
        assert res is vis
        save(f"visops_to_stokes_{frame}.npz", **inp, **outputs(res, ""))

    for i, frame in enumerate(("linear", "linearnp", "circular", "circularnp")):
        vis = base_case(frame, 66 + i)
        inp = inputs(vis, frame)
        res = ns["convert_visibility_to_stokesI"](vis)
        assert res is not vis and res.vis.shape[3] == 1
        save(f"visops_to_stokesI_{frame}.npz", **inp, **outputs(res, ""))

    vis = base_case("stokesI", 70)
    inp = inputs(vis, "stokesI")
    res = ns["convert_visibility_stokesI_to_polframe"](vis, dm.PolarisationFrame("linear"))
    save("visops_polframe_linear.npz", **inp, **outputs(res, ""))

    vis = base_case("linear", 71, continuum=True)
    out = inputs(vis, "linear")
    mask = np.zeros(8, dtype=bool)
    mask[list(MASK_CHANNELS)] = True
    out["mask"] = mask
    fw = vis["weight"].data * (1 - vis["flags"].data)
    for tag, degree, m in (("deg0", 0, None), ("deg1", 1, None), ("deg2", 2, None),
                           ("deg1_mask", 1, mask)):
        w = fw.copy()
        if m is not None:
            w[:, :, m, :] = 0.0
        live = (w != 0).sum(axis=2)
        assert live.min() >= 1, "the reference raises on a spectrum without weight"
        deficient = np.argwhere(live.reshape(-1) <= degree).reshape(-1)
        out[f"deficient_{tag}"] = deficient
        print(tag, "rank-deficient spectra:", deficient.tolist())
        v = vis.copy(deep=True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ns["remove_continuum_visibility"](v, degree=degree, mask=m)
        assert res is v
        out[f"out_vis_{tag}"] = np.asarray(res["vis"].data)
    save("visops_continuum_linear.npz", **out)


if __name__ == "__main__":
    main()
