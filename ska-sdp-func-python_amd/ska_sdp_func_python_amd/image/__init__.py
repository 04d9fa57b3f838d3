"""Image-plane stages after the invert: CLEAN deconvolution and restore, and
the scatter and gather of images by facet and by channel."""

from . import (  # noqa: F401
    cleaners,
    deconvolution,
    gather_scatter,
    iterators,
    operations,
    taylor_terms,
)
from .deconvolution import (  # noqa: F401
    deconvolve_cube,
    deconvolve_list,
    fit_psf,
    restore_cube,
    restore_list,
)
from .gather_scatter import (  # noqa: F401
    image_gather_channels,
    image_gather_facets,
    image_scatter_channels,
    image_scatter_facets,
)
from .iterators import image_channel_iter, image_raster_iter  # noqa: F401
