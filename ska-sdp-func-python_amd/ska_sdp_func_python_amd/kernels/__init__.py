"""Tensor-level wrappers over the C ABI (device buffers are torch tensors).

These are the thin host shims between the reference-shaped Python API
(imaging/, calibration/, grid_data/) and libska_sdp_hip.so.  They validate
shapes, dtypes and devices, pass raw device pointers + element strides, and
enqueue on torch's current HIP stream.  Nothing here computes on the CPU.

One module per kernel family, named after its csrc file; ``_operands`` holds
what they share.  Callers use the names re-exported here
(``kernels.ms2dirty(...)``), looked up at call time, so that a test or a
benchmark can put a stand-in on the package.
"""

from .. import _lib  # noqa: F401
from ._operands import (DT_CODE, FLAG_BYTES, alloc, byte_ranges, check_uvw, dev_array,  # noqa: F401
                        f64_like, flags_of, host_doubles, on_gpu, overlaps, plane_list, ptr,
                        ptr_table, stream, vis4)
from .wgrid import (EPS_FLOOR, dirty2ms, dirty2ms_vis, dirty2ms_vis_pols, is_fp64,  # noqa: F401
                    layout_fingerprint, merge_bounds, ms2dirty, ms2dirty_batch, ms2dirty_vis,
                    ms2dirty_vis_pols, release_workspace, set_precision, set_stage_timing,
                    uvw_bounds, wstack_layout)
from .dft import dft_point, idft_point  # noqa: F401
from .cfgrid import degrid_cf, grid_cf  # noqa: F401
from .weighting import WEIGHTING, grid_weights, reweight, taper  # noqa: F401
from .calops import (GAIN_CHAIN_MAX, apply_gain_chain, apply_gains, canonical_baselines,  # noqa: F401
                     divide_vis, point_sums, solve_gains)
from .visops import (MAX_CONTINUUM_DEGREE, vis_average_channels, vis_remove_continuum,  # noqa: F401
                     vis_to_stokes, vis_to_stokes_i)
from .clean import CLEAN_STOP, clean_plane, clean_plane_complex, mfsclean_plane  # noqa: F401
from .skycomp import (RESTORE_SKIP_ARGUMENT, SKYCOMP_MAX_PAIRS, skycomp_insert,  # noqa: F401
                      skycomp_nearest, skycomp_restore, tile_boxes, tile_csr)
from .planes import (MIX_NAN_INPUT, MIX_NAN_OUTPUT, MIX_PLANES_MAX, MIX_PLANES_REGS,  # noqa: F401
                     PEAK_NAN_INPUT, PEAK_NAN_MEAN, SUM_PLANES_MAX, mix_planes, peak_abs,
                     sum_planes)
from .facets import GATHER_FACETS_MAX, gather_facet_weights, gather_facets  # noqa: F401
from .segment import SEGMENT_KERNEL_MAX, segment_image, segment_peaks  # noqa: F401
from .gaussfit import GAUSS_FIT_STATUS, GAUSS_FIT_WINDOW, gauss_fit  # noqa: F401
from .bandpass import (BANDPASS_MAX_DEGREE, BANDPASS_MAX_SEGMENTS, resample_interp,  # noqa: F401
                       resample_polyfit)
from .wkernel import wkernel_create  # noqa: F401
