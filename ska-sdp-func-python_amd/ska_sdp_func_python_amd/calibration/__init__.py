"""Calibration: solve_gaintable (batched StefCal on MI355X), apply_gaintable,
chains of gain tables (calibrate_chain, solve_calibrate_chain,
apply_calibration_chain), gain-table operations and the CBF beamformer
utilities (bandpass resampling on the GPU)."""
from .beamformer_utils import (  # noqa: F401
    expand_delay_phase,
    multiply_gaintable_jones,
    resample_bandpass,
    set_beamformer_frequencies,
)
from .chain_calibration import (  # noqa: F401
    apply_calibration_chain,
    calibrate_chain,
    create_calibration_controls,
    solve_calibrate_chain,
)
from .jones import apply_jones  # noqa: F401
from .operations import (  # noqa: F401
    apply_gaintable,
    concatenate_gaintables,
    multiply_gaintables,
)
from .solvers import solve_gaintable  # noqa: F401
