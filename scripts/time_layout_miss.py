"""The C2 invert's cacheable miss and the layout's first two hits: one uvw
element changes in place before every round, so its first call plans afresh
and keeps its layout; the second call is the first hit (which records the
permutation, unless SDP_HIP_LAYOUT_RECORD=1 had the miss do it) and the third
a replay.  Prints the median times of the three calls and the miss's median
ms_prep, one stream; run it once per library build (SDP_HIP_LIB_OVERRIDE) and
alternate the builds.
usage: python3 scripts/time_layout_miss.py [steps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "ska-sdp-func-python_amd"))
import numpy as np
import torch
from ska_sdp_func_python_amd import kernels, simulation

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
dev = torch.device("cuda:0")
obs = simulation.device_observation(100, 64, 0.95e9, 1.76e9, config="MID", seed=0, device=dev)
cell = 0.25 / obs["umax"]
sw = torch.zeros(1, dtype=torch.float64, device=dev)
vis3 = obs["vis"].unsqueeze(2)


def call():
    return kernels.ms2dirty_vis(obs["uvw"], obs["freq"], vis3, 0, obs["wgt"], None, None, 4096,
                                4096, cell, cell, 1e-7, True, flip_uw=True, sumwt=sw)[1]


row = obs["uvw"].shape[0] // 2
base = float(obs["uvw"][row, 1])
def timed_call():
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    info = call()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, info


# each round: a miss (new uvw content), then the layout's first and second hit
ms, prep, hit1, hit2, flags = [], [], [], [], []
for timing in (False, True):
    kernels.set_stage_timing(timing)
    for i in range(steps + 2):
        obs["uvw"][row, 1] = base * (1.0 + 1e-9 * (i + 1 + (100 if timing else 0)))
        t_miss, info = timed_call()
        t_h1, i1 = timed_call()
        t_h2, i2 = timed_call()
        if i >= 2:
            flags.append((info["layout_reused"], i1["layout_reused"], i2["layout_reused"]))
            if timing:
                prep.append(info["ms_prep"])
            else:
                ms.append(t_miss)
                hit1.append(t_h1)
                hit2.append(t_h2)
assert all(f == (0, 1, 1) for f in flags), flags
print(json.dumps({"lib": os.environ.get("SDP_HIP_LIB_OVERRIDE", "cur"),
                  "record": os.environ.get("SDP_HIP_LAYOUT_RECORD", "0"),
                  "ms_miss_step": round(float(np.median(ms)), 3),
                  "ms_miss_step_min_max": [round(min(ms), 3), round(max(ms), 3)],
                  "ms_prep_miss": round(float(np.median(prep)), 3),
                  "ms_first_hit": round(float(np.median(hit1)), 3),
                  "ms_second_hit": round(float(np.median(hit2)), 3)}))
