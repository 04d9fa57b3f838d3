"""Sky-component operations: the beam helper of the sky-model drivers, the
image-side operations (insert, restore, Voronoi) and the frequency Taylor
terms of component lists."""
from .operations import (  # noqa: F401
    apply_beam_to_skycomponent,
    image_voronoi_iter,
    insert_skycomponent,
    restore_skycomponent,
    voronoi_decomposition,
)
from .taylor_terms import (  # noqa: F401
    calculate_skycomponent_list_taylor_terms,
    gather_skycomponents_from_channels,
    interpolate_skycomponents_frequency,
    transpose_skycomponents_to_channels,
)
