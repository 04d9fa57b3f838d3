"""FFT support functions (reference src/ska_sdp_func_python/fourier_transforms):
centred transforms, padding and extraction, FFT coordinates, the spheroidal
function and the w beam."""

from .fft_coordinates import *  # noqa: F401,F403
from .fft_support import *  # noqa: F401,F403
