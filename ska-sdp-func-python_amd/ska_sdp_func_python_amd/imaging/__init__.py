"""Imaging hot path: predict/invert (w-stacking NUFFT), the sky-component DFT and imaging weights."""
from .base import (advise_wide_field, create_image_from_visibility, normalise_sumwt,  # noqa: F401
                   rad_deg_arcsec, shift_vis_to_image, visibility_recentre)
from .dft import (dft_skycomponent_visibility, extract_direction_and_flux,  # noqa: F401
                  idft_visibility_skycomponent)
from .imaging import invert_visibility, predict_visibility  # noqa: F401
from .imaging_helpers import (remove_sumwt, sum_invert_results, sum_predict_results,  # noqa: F401
                              threshold_list)
from .ng import invert_ng, predict_ng  # noqa: F401
from .weighting import (taper_visibility_gaussian, taper_visibility_tukey,  # noqa: F401
                        weight_visibility)
from .wg import invert_wg, predict_wg  # noqa: F401
