"""apply_jones (reference ``src/ska_sdp_func_python/calibration/jones.py:8-27``):
a 2x2 Jones matrix, or its inverse, on both sides of a 2x2 coherency matrix.
Host numpy, as in the reference: one matrix at a time is no GPU work.
"""

import numpy as np


def apply_jones(ej, cfs, inverse=False, min_det=1e-6):
    """ej cfs ej^H, or ej^-1 cfs ej^-H with ``inverse``; where |det ej| does
    not exceed ``min_det`` the inverse gives zeros shaped like ``cfs``."""
    if not inverse:
        return ej @ cfs @ np.conjugate(ej).T
    if np.abs(np.linalg.det(ej)) > min_det:
        inv = np.linalg.inv(ej)
        return inv @ cfs @ np.conjugate(inv).T
    return 0.0 * cfs
