"""Sky-component operations: the beam helper of the sky-model drivers and the
image-side operations (insert, restore, Voronoi)."""
from .operations import (  # noqa: F401
    apply_beam_to_skycomponent,
    image_voronoi_iter,
    insert_skycomponent,
    restore_skycomponent,
    voronoi_decomposition,
)
