"""Generate the inverse-DFT golden fixtures tests/golden/idft_*.npz from the
REFERENCE's own code.

Run in the build container only (needs the reference checkout, see
make_golden.py):  python tests/golden/make_golden_idft.py

The reference's idft_visibility_skycomponent (imaging/dft.py:340-387) and
calculate_visibility_phasor (visibility/base.py:27-45) are AST-extracted and
executed with numpy on the datamodels shim, as make_golden.py does.  Only
inputs and outputs are stored -- no reference source text.

One visibility set per case: simulation.make_visibility("LOW"), 8 antennas,
2 times, 3 channels; the visibilities are the reference's dft_cpu_looped of 3
components plus noise; weights uniform(0.5, 2), about 10% of the samples
flagged and one (channel, pol) flagged entirely, so that its summed weight
is 0 and the flux there must be exactly 0.

Cases:
  idft_linear_iquv.npz   linear visibilities, stokesIQUV components
                         (the flux is converted back from linear)
  idft_circular.npz      circular visibilities, circular components
  idft_stokesI_single.npz  stokesI visibilities, ONE component passed bare
                         (not in a list)
"""

import collections.abc
import os
import sys
from typing import List, Union

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import dm, load_reference, save, simulation  # noqa: E402

from ska_sdp_func_python_amd.util.coordinate_support import skycoord_to_lmn  # noqa: E402


def _reference():
    base = load_reference("visibility/base.py", ["calculate_visibility_phasor"],
                          {"skycoord_to_lmn": skycoord_to_lmn})
    idft = load_reference(
        "imaging/dft.py", ["idft_visibility_skycomponent", "dft_cpu_looped"],
        {"calculate_visibility_phasor": base["calculate_visibility_phasor"],
         "convert_pol_frame": dm.convert_pol_frame, "collections": collections,
         "Union": Union, "List": List, "SkyComponent": dm.SkyComponent})
    return idft


def make_case(ns, tag, vis_frame, comp_frame, single, seed):
    rng = np.random.default_rng(seed)
    pc = dm.SkyCoord(180.0, -35.0, unit="deg")
    vis = simulation.make_visibility("LOW", nants=8, ntimes=2, nchan=3, f_lo=1.0e8, f_hi=1.1e8,
                                     polarisation_frame=vis_frame, phasecentre=pc)
    vpf = vis.visibility_acc.polarisation_frame
    cpf = dm.PolarisationFrame(comp_frame)
    nchan, npol = 3, vpf.npol
    ncomp = 1 if single else 3
    radec = np.stack([180.0 + rng.uniform(-1.0, 1.0, ncomp), -35.0 + rng.uniform(-1.0, 1.0, ncomp)], 1)
    cflux = rng.uniform(1.0, 10.0, (ncomp, nchan, cpf.npol))
    if cpf.npol > 1:
        cflux[..., 1:] *= 0.1
    comps = [dm.SkyComponent(dm.SkyCoord(ra, dec, unit="deg"), vis.frequency.data, flux=cflux[i],
                             polarisation_frame=cpf) for i, (ra, dec) in enumerate(radec)]
    # visibilities: the reference's forward DFT of the components plus noise
    dcs, vfl = [], []
    for comp in comps:
        l, m, _ = skycoord_to_lmn(comp.direction, pc)
        dcs.append([l, m, np.sqrt(1 - l ** 2 - m ** 2) - 1.0])
        vfl.append(dm.convert_pol_frame(comp.flux, cpf, vpf))
    uvw_lambda = np.asarray(vis.visibility_acc.uvw_lambda)
    v = ns["dft_cpu_looped"](np.array(dcs), uvw_lambda, np.array(vfl).astype(complex))
    shape = v.shape
    v = v + 0.05 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    weight = rng.uniform(0.5, 2.0, shape)
    flags = (rng.uniform(size=shape) < 0.1).astype(int)
    flags[:, :, 1, npol - 1] = 1  # one (channel, pol) without any weight
    vis["vis"].data = v
    vis["weight"].data = weight
    vis["flags"].data = flags
    newsc, weights = ns["idft_visibility_skycomponent"](vis, comps[0] if single else comps)
    assert len(newsc) == ncomp and len(weights) == ncomp
    w = np.array(weights)
    assert np.all(w[:, 1, npol - 1] == 0)
    save(f"idft_{tag}.npz", uvw=np.asarray(vis.uvw.data), frequency=np.asarray(vis.frequency.data),
         channel_bandwidth=np.asarray(vis.channel_bandwidth.data), time=np.asarray(vis.time.data),
         integration_time=np.asarray(vis.integration_time.data),
         baselines=np.asarray(vis.baselines.data), phasecentre_deg=np.array([180.0, -35.0]),
         vis=v, weight=weight, flags=flags, vis_frame=np.array(vis_frame),
         comp_frame=np.array(comp_frame), comp_radec_deg=radec, comp_flux=cflux,
         single=np.array(int(single)), flux=np.array([c.flux for c in newsc]), weights=w)


def main():
    ns = _reference()
    make_case(ns, "linear_iquv", "linear", "stokesIQUV", False, 21)
    make_case(ns, "circular", "circular", "circular", False, 22)
    make_case(ns, "stokesI_single", "stokesI", "stokesI", True, 23)


if __name__ == "__main__":
    main()
