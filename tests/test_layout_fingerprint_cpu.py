"""The content fingerprint an invert keeps its bucketing layout under
(csrc/wstack_fingerprint.h through sdp_hip_wstack_fingerprint: host arrays, no
device work): deterministic, independent of the row stride, and not blind to
the order of the content -- swapping two rows, or moving a value to another
row, changes it, although every word is an order-independent sum."""

import numpy as np


def _data(seed=5, nrow=257, nchan=9):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(nrow, 3)) * 1.0e3, np.linspace(1.0e9, 1.3e9, nchan)


def test_deterministic_and_content_only():
    from ska_sdp_func_python_amd import kernels
    uvw, freq = _data()
    a = kernels.layout_fingerprint(uvw, freq)
    assert a == kernels.layout_fingerprint(uvw.copy(), freq.copy())
    assert len(a) == 4 and all(0 <= w < 2 ** 64 for w in a) and len(set(a)) == 4
    # a padded row stride holds the same content
    wide = np.zeros((uvw.shape[0], 5))
    wide[:, :3] = uvw
    assert kernels.layout_fingerprint(wide[:, :3], freq) == a
    # the uvw words do not depend on freq, nor the freq words on uvw
    b = kernels.layout_fingerprint(uvw, freq * 2.0)
    assert b[:2] == a[:2] and b[2] != a[2] and b[3] != a[3]


def test_every_element_counts():
    from ska_sdp_func_python_amd import kernels
    uvw, freq = _data()
    a = kernels.layout_fingerprint(uvw, freq)
    for r, c in ((0, 0), (100, 1), (256, 2)):
        x = uvw.copy()
        x[r, c] = np.nextafter(x[r, c], np.inf)  # one bit
        f = kernels.layout_fingerprint(x, freq)
        assert f[0] != a[0] and f[1] != a[1] and f[2:] == a[2:]
    g = freq.copy()
    g[4] = np.nextafter(g[4], np.inf)
    f = kernels.layout_fingerprint(uvw, g)
    assert f[:2] == a[:2] and f[2] != a[2] and f[3] != a[3]
    # -0.0 and 0.0 are different bit patterns
    z = uvw.copy()
    z[7, 2] = 0.0
    zn = z.copy()
    zn[7, 2] = -0.0
    assert kernels.layout_fingerprint(z, freq) != kernels.layout_fingerprint(zn, freq)
    # a row more is another content
    assert kernels.layout_fingerprint(uvw[:-1], freq)[:2] != a[:2]


def test_not_blind_to_order():
    from ska_sdp_func_python_amd import kernels
    uvw, freq = _data()
    a = kernels.layout_fingerprint(uvw, freq)
    sw = uvw.copy()
    sw[[10, 200]] = sw[[200, 10]]            # two rows swapped
    f = kernels.layout_fingerprint(sw, freq)
    assert f[0] != a[0] and f[1] != a[1]
    mv = uvw.copy()
    mv[10, 0], mv[11, 0] = uvw[11, 0], uvw[10, 0]  # a value moved to another row
    f = kernels.layout_fingerprint(mv, freq)
    assert f[0] != a[0] and f[1] != a[1]
    col = uvw.copy()
    col[10, 0], col[10, 1] = uvw[10, 1], uvw[10, 0]  # ... or to another column
    f = kernels.layout_fingerprint(col, freq)
    assert f[0] != a[0] and f[1] != a[1]
    assert kernels.layout_fingerprint(uvw, freq[::-1].copy())[2:] != a[2:]
    # equal rows at different indices are different terms: duplicating the
    # content does not double (or cancel) the sums
    two = np.concatenate([uvw[:4], uvw[:4]])
    one = kernels.layout_fingerprint(uvw[:4], freq)
    f2 = kernels.layout_fingerprint(two, freq)
    assert f2[0] != (2 * one[0]) % 2 ** 64 and f2[0] != one[0]
