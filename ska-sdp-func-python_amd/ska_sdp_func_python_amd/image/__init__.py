"""Image-plane stages after the invert: CLEAN deconvolution and restore."""

from . import cleaners, deconvolution, operations, taylor_terms  # noqa: F401
from .deconvolution import (  # noqa: F401
    deconvolve_cube,
    deconvolve_list,
    fit_psf,
    restore_cube,
    restore_list,
)
