"""predict_wg / invert_wg (reference src/ska_sdp_func_python/imaging/wg.py):
the ``context="wg"`` entry points, which in the reference call the WAGG GPU
gridder with the arguments and the u, w flips of the nifty-gridder functions.
Here both contexts run on the same HIP w-stacking NUFFT, so the two functions
check what the reference checks and delegate to ``predict_ng`` / ``invert_ng``.

    predict_wg  (:35-154)   ValueError for a non-canonical model and for a
                            model whose polarisations do not match the
                            visibility's
    invert_wg   (:157-303)  ValueError for a non-canonical model

Kwargs ``epsilon`` (default 1e-12) and ``do_wstacking`` (True) are passed on;
``threads`` and ``verbosity`` are accepted and ignored.

One deviation: the reference returns ``None`` from either function when the
``wagg`` module cannot be imported.  There is no such module to miss here, so
neither function ever returns ``None`` for that reason.
"""

import logging

from .ng import invert_ng, predict_ng

__all__ = ["invert_wg", "predict_wg"]

log = logging.getLogger("func-python-logger")


def _check_canonical(model):
    if not model.image_acc.is_canonical():
        log.error("The image model is not canonical. See the logfile. Exiting...")
        raise ValueError("WG:The image model is not canonical")


def _ng_kwargs(kwargs):
    return {k: v for k, v in kwargs.items() if k not in ("threads", "verbosity")}


def predict_wg(bvis, model, **kwargs):
    """Predict using convolutional degridding (reference wg.py:35).

    :param bvis: Visibility to be predicted
    :param model: Model Image
    :return: Resulting Visibility (never None: see the module's note)
    """
    _check_canonical(model)
    if model["pixels"].data.shape[1] != bvis.vis.shape[3]:
        log.error("The number of polarisations in bvis and a model does not match, exiting...")
        raise ValueError("WG: The number of polarisations in bvis and a model does not match")
    return predict_ng(bvis, model, **_ng_kwargs(kwargs))


def invert_wg(bvis, model, dopsf=False, normalise=True, **kwargs):
    """Invert to a dirty image or PSF (reference wg.py:157).

    :param bvis: Visibility to be inverted
    :param model: Image template (not changed)
    :param dopsf: Make the PSF instead of the dirty image
    :param normalise: Normalise by the sum of weights (True)
    :return: (resulting Image, sum of the weights for each frequency and
             polarisation); never None: see the module's note
    """
    _check_canonical(model)
    return invert_ng(bvis, model, dopsf=dopsf, normalise=normalise, **_ng_kwargs(kwargs))
