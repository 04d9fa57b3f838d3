"""Sky-component operations: the beam helper of the sky-model drivers, the
image-side operations (insert, restore, Voronoi, find), the catalogue helpers
and the frequency Taylor terms of component lists."""
from .operations import (  # noqa: F401
    apply_beam_to_skycomponent,
    filter_skycomponents_by_flux,
    find_nearest_skycomponent,
    find_nearest_skycomponent_index,
    find_separation_skycomponents,
    find_skycomponent_matches,
    find_skycomponent_matches_atomic,
    find_skycomponents,
    fit_skycomponent,
    fit_skycomponent_spectral_index,
    fit_skycomponents,
    image_voronoi_iter,
    insert_skycomponent,
    partition_skycomponent_neighbours,
    remove_neighbouring_components,
    restore_skycomponent,
    segment_image,
    select_components_by_separation,
    select_neighbouring_components,
    voronoi_decomposition,
)
from .taylor_terms import (  # noqa: F401
    calculate_skycomponent_list_taylor_terms,
    find_skycomponents_frequency_taylor_terms,
    gather_skycomponents_from_channels,
    interpolate_skycomponents_frequency,
    transpose_skycomponents_to_channels,
)
