"""Visibility helpers on the hot path (reference src/ska_sdp_func_python/visibility/)."""
from .base import calculate_visibility_phasor, phaserotate_visibility  # noqa: F401
from .operations import (average_visibility_by_channel, concatenate_visibility,  # noqa: F401
                         concatenate_visibility_frequency, convert_visibility_stokesI_to_polframe,
                         convert_visibility_to_stokes, convert_visibility_to_stokesI,
                         divide_visibility, expand_polarizations,
                         integrate_visibility_by_channel, remove_continuum_visibility,
                         subtract_visibility)
