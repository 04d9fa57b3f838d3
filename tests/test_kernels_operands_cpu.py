"""The kernels package's public surface and its shared operand helpers
(kernels/_operands.py, the w-gridder's coef packing), on the host."""

import ctypes
import gc

import numpy as np
import pytest
import torch

# every public name of the flat kernels module this package replaced: the contract
SURFACE = """
EPS_FLOOR WEIGHTING GAIN_CHAIN_MAX MAX_CONTINUUM_DEGREE CLEAN_STOP SKYCOMP_MAX_PAIRS
RESTORE_SKIP_ARGUMENT MIX_PLANES_REGS MIX_PLANES_MAX MIX_NAN_INPUT MIX_NAN_OUTPUT
GATHER_FACETS_MAX SEGMENT_KERNEL_MAX GAUSS_FIT_WINDOW GAUSS_FIT_STATUS BANDPASS_MAX_DEGREE
BANDPASS_MAX_SEGMENTS SUM_PLANES_MAX PEAK_NAN_INPUT PEAK_NAN_MEAN
set_precision is_fp64 ms2dirty ms2dirty_batch ms2dirty_vis ms2dirty_vis_pols dirty2ms
dirty2ms_vis dirty2ms_vis_pols uvw_bounds merge_bounds wstack_layout layout_fingerprint
set_stage_timing release_workspace dft_point idft_point grid_cf degrid_cf grid_weights
reweight taper canonical_baselines solve_gains point_sums divide_vis apply_gains
apply_gain_chain vis_average_channels vis_to_stokes vis_to_stokes_i vis_remove_continuum
clean_plane clean_plane_complex mfsclean_plane skycomp_insert skycomp_restore
skycomp_nearest mix_planes sum_planes peak_abs gather_facets gather_facet_weights
segment_image segment_peaks gauss_fit resample_polyfit resample_interp
""".split()
# the helpers that used to be reached by a private name, and the library handle
SHARED = """on_gpu ptr stream alloc DT_CODE dev_array FLAG_BYTES flags_of f64_like host_doubles
ptr_table plane_list byte_ranges overlaps tile_boxes tile_csr _lib""".split()


def _doubles(p, n):
    return ctypes.cast(p, ctypes.POINTER(ctypes.c_double))[:n]


def test_the_package_keeps_the_flat_modules_public_names():
    from ska_sdp_func_python_amd import kernels
    missing = [name for name in SURFACE + SHARED if not hasattr(kernels, name)]
    assert not missing, missing


def test_flag_bytes_is_the_one_table():
    from ska_sdp_func_python_amd import kernels
    assert kernels.FLAG_BYTES == {torch.int64: 8, torch.int32: 4, torch.int8: 1, torch.uint8: 1,
                                  torch.bool: 1}


def test_coef_packs_interleaved_and_row_major():
    from ska_sdp_func_python_amd.kernels import wgrid
    assert wgrid._coef_buffer(None, None, 2) is None and wgrid._coef_buffer(None, 2, 2) is None
    vec = wgrid._coef_buffer([1 + 2j, 3 - 4j], None, 2)
    mat = wgrid._coef_buffer([[1, 2j], [3 + 4j, -5]], 2, 2)
    gc.collect()
    assert _doubles(vec, 4) == [1.0, 2.0, 3.0, -4.0]
    assert _doubles(mat, 8) == [1.0, 0.0, 0.0, 2.0, 3.0, 4.0, -5.0, 0.0]
    with pytest.raises(ValueError):
        wgrid._coef_buffer([1, 2, 3], None, 2)
    with pytest.raises(ValueError):
        wgrid._coef_buffer([[1, 2], [3]], 2, 2)
    with pytest.raises(ValueError):
        wgrid._coef_buffer([[1, 2]], 2, 2)


def test_host_buffers_outlive_their_makers():
    """The bare pointers own their arrays: the contents are still there after
    a collection, with nothing else holding them."""
    from ska_sdp_func_python_amd import kernels
    p = kernels.host_doubles(iter([0.25, -1.5, 3.0]))
    a, b = torch.arange(3.0), torch.arange(5.0)
    tab = kernels.ptr_table([a, b])
    junk = [kernels.host_doubles([9.0] * 3) for _ in range(64)]  # would reuse a freed block
    del junk
    gc.collect()
    assert _doubles(p, 3) == [0.25, -1.5, 3.0]
    assert ctypes.cast(tab, ctypes.POINTER(ctypes.c_void_p))[:3] == [a.data_ptr(), b.data_ptr(),
                                                                   None]
    assert kernels.host_doubles(None) is None
    assert _doubles(kernels.host_doubles([1.0], 3), 3) == [1.0, 0.0, 0.0]


def test_overlaps_is_half_open():
    from ska_sdp_func_python_amd import kernels
    u = lambda *v: np.array(v, dtype=np.uint64)
    # [0, 8) against: [8, 16) touching, [32, 40) disjoint, [2, 4) nested, [4, 12) straddling
    got = kernels.overlaps(u(0), u(8), u(8, 32, 2, 4), u(16, 40, 4, 12))
    assert got.tolist() == [False, False, True, True]
    assert kernels.overlaps(u(2), u(4), u(0), u(8)).all()  # nested the other way round


def test_flags_of_and_f64_like_refuse_host_tensors():
    from ska_sdp_func_python_amd import kernels
    vis = torch.zeros((2, 3, 4, 1), dtype=torch.complex64)
    assert kernels.flags_of(None, vis.shape) == (None, 0)
    with pytest.raises(ValueError, match=r"flags must be a device \(HIP\) tensor"):
        kernels.flags_of(torch.zeros(vis.shape, dtype=torch.int32), vis.shape)
    with pytest.raises(ValueError, match=r"weight must be a device \(HIP\) tensor"):
        kernels.f64_like(torch.zeros(vis.shape, dtype=torch.float64), "weight", vis)
    with pytest.raises(ValueError, match=r"weight must be a device \(HIP\) tensor"):
        kernels.f64_like(None, "weight", vis)
