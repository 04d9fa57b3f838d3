"""The identity the invert's Hermitian fold rests on (csrc/wstack_types.h,
Geo::fold), pinned on the CPU with the exact direct sums: the dirty image is
the real part of the transform, so a visibility at (u, v, w) and its conjugate
at (-u, -v, -w) contribute the same image.  Expected difference 0; bound
1e-14 relative RMS (a few fp64 roundings of a sum of order-1 terms)."""

import numpy as np
import pytest

import nufft_oracle as orc
from conftest import rel_rms


@pytest.mark.parametrize("dow", [False, True])
def test_folded_input_gives_the_same_exact_image(dow):
    rng = np.random.default_rng(21)
    nrow, nchan, umax = 300, 3, 2000.0
    freq = np.linspace(1.0e9, 1.2e9, nchan)
    uvw = rng.uniform(-1, 1, (nrow, 3)) * umax * orc.C_LIGHT / freq.max()
    uvw[:, 2] *= 12.0
    uvw[:3, 0] = 0.0  # u = 0 does not fold
    ms = rng.normal(size=(nrow, nchan)) + 1j * rng.normal(size=(nrow, nchan))
    wgt = rng.uniform(0.5, 1.5, (nrow, nchan))
    cell = 0.45 / umax
    fold = uvw[:, 0] < 0
    assert 100 < fold.sum() < 200
    fuvw = np.where(fold[:, None], -uvw, uvw)
    fms = np.where(fold[:, None], ms.conj(), ms)
    assert (fuvw[:, 0] >= 0).all()
    ref = orc.ms2dirty_exact(uvw, freq, ms, wgt, 64, 48, cell, cell * 0.9, dow)
    got = orc.ms2dirty_exact(fuvw, freq, fms, wgt, 64, 48, cell, cell * 0.9, dow)
    assert rel_rms(got, ref) < 1e-14
