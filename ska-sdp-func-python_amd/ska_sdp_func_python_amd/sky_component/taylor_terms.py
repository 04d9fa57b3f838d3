"""Frequency Taylor terms of sky-component lists (reference
src/ska_sdp_func_python/sky_component/taylor_terms.py:32-80, :156-241), on the
host: the work is O(components x channels).

    calculate_skycomponent_list_taylor_terms   flux decoupled into Taylor terms
                                               with pinv of the coupling matrix
    interpolate_skycomponents_frequency        flux smoothed by a polynomial fit
    transpose_skycomponents_to_channels        [source] -> [chan][source]
    gather_skycomponents_from_channels         [chan][source] -> [source]

The weights are w_k = ((nu - nu_ref) / nu_ref) ** k as for images
(image/taylor_terms.py), with ``numpy.linalg.pinv(coupling, rcond=1e-7)`` and
``numpy.polynomial.polynomial.polyfit`` / ``polyval`` as in the reference.

``find_skycomponents_frequency_taylor_terms`` (:83-153) joins the device
functions: moment 0 of the channel images (image/taylor_terms.py),
``find_skycomponents`` on it and one batch of Gaussian fits, every component
in every channel image (``fit_skycomponents``), then the two host functions
above.
"""

import logging

import numpy
from numpy.polynomial import polynomial

__all__ = ["calculate_skycomponent_list_taylor_terms",
           "find_skycomponents_frequency_taylor_terms",
           "gather_skycomponents_from_channels",
           "interpolate_skycomponents_frequency",
           "transpose_skycomponents_to_channels"]

log = logging.getLogger("func-python-logger")


def calculate_skycomponent_list_taylor_terms(sc_list, nmoment=1, reference_frequency=None):
    """Frequency Taylor terms of a list of SkyComponents.

    :param sc_list: list of SkyComponents, flux [nchan, npol]
    :param nmoment: number of Taylor terms
    :param reference_frequency: reference frequency (default: the centre channel's)
    :return: per component, a list of ``nmoment`` SkyComponents at the reference
        frequency, flux [1, npol]; ``[[]]`` for an empty list
    """
    if len(sc_list) == 0:
        return [nmoment * []]
    nchan = len(sc_list[0].frequency)
    if reference_frequency is None:
        reference_frequency = sc_list[0].frequency[len(sc_list[0].frequency) // 2]
    log.debug("calculate_image_from_frequency_moments: Reference frequency = %.3f (MHz)",
              1e-6 * reference_frequency)

    channel_moment_coupling = numpy.zeros([nchan, nmoment])
    for chan in range(nchan):
        for m in range(nmoment):
            channel_moment_coupling[chan, m] += numpy.power(
                (sc_list[0].frequency[chan] - reference_frequency) / reference_frequency, m)
    pinv = numpy.linalg.pinv(channel_moment_coupling, rcond=1e-7)

    newsc_list = []
    for sc in sc_list:
        taylor_term_sc_list = []
        for moment in range(nmoment):
            taylor_term_data = numpy.zeros([1, sc.polarisation_frame.npol])
            for chan in range(nchan):
                # (the reference adds flux[chan, 0], Stokes I, to every polarisation)
                taylor_term_data[0] += pinv[moment, chan] * sc.flux[chan, 0]
            taylor_term_sc = sc.copy()
            taylor_term_sc.flux = taylor_term_data
            taylor_term_sc.frequency = reference_frequency
            taylor_term_sc_list.append(taylor_term_sc)
        newsc_list.append(taylor_term_sc_list)
    return newsc_list


def find_skycomponents_frequency_taylor_terms(dirty_list, nmoment=1, reference_frequency=None,
                                              **kwargs):
    """Find components in moment 0 of a list of channel images, fit each in
    every channel, smooth the fluxes by a polynomial in frequency and return
    them per channel (reference :83-153).

    The components are those of ``find_skycomponents`` on the moment-0 image,
    above ``component_threshold`` (default: infinity, which finds none).  Each
    gets, per channel image, the Stokes fluxes ``fit_skycomponent(image,
    component).flux[0, :]``; all of these fits run as one batch on the device.

    :param dirty_list: list of single-channel Images at different frequencies
    :param nmoment: number of polynomial terms fitted in frequency
    :param reference_frequency: reference frequency (default: the centre image's)
    :param component_threshold: threshold of the search in moment 0
    :return: list over channels of lists of single-channel SkyComponents; ``[]``
        when no component is found
    """
    from ..image.taylor_terms import calculate_frequency_taylor_terms_from_image_list
    from .operations import find_skycomponents, fit_skycomponents
    frequency = numpy.array([d.frequency[0] for d in dirty_list])
    if reference_frequency is None:
        reference_frequency = frequency[len(frequency) // 2]
    log.debug("find_skycomponents_frequency_taylor_terms: Reference frequency = %.3f (MHz)",
              1e-6 * reference_frequency)

    moment0_list = calculate_frequency_taylor_terms_from_image_list(
        dirty_list, nmoment=1, reference_frequency=reference_frequency)
    threshold = kwargs.get("component_threshold", numpy.inf)
    try:
        moment0_skycomponents = find_skycomponents(moment0_list[0], threshold=threshold)
    except ValueError:
        log.info("find_skycomponents_frequency_taylor_terms: No skycomponents found in moment 0")
        return []
    ncomps = len(moment0_skycomponents)
    if ncomps == 0:
        return []
    log.info("find_skycomponents_frequency_taylor_terms: found %s skycomponents in moment 0",
             ncomps)

    fit_kwargs = {k: v for k, v in kwargs.items() if k != "component_threshold"}
    fitted = fit_skycomponents(dirty_list, moment0_skycomponents, **fit_kwargs)
    found_component_list = []
    for isc, sc in enumerate(moment0_skycomponents):
        found_component = sc.copy()
        found_component.frequency = frequency
        found_component.flux = numpy.array([list(fitted[chan][isc].flux[0, :])
                                            for chan in range(len(dirty_list))])
        found_component_list.append(found_component)
        log.info("Component %s: %s", isc, found_component)

    interpolated_sc_list = interpolate_skycomponents_frequency(
        found_component_list, nmoment=nmoment, reference_frequency=reference_frequency)
    return transpose_skycomponents_to_channels(interpolated_sc_list)


def interpolate_skycomponents_frequency(sc_list, nmoment=1, reference_frequency=None):
    """SkyComponent fluxes smoothed by a polynomial of ``nmoment`` terms in
    (nu - nu_ref) / nu_ref, fitted per component and polarisation.

    :param sc_list: list of SkyComponents on the frequencies of the first
    :param nmoment: number of polynomial terms
    :param reference_frequency: reference frequency (default: the centre channel's)
    :return: list of interpolated SkyComponents
    """
    frequency = sc_list[0].frequency
    if reference_frequency is None:
        reference_frequency = frequency[len(frequency) // 2]
    log.debug("interpolate_skycomponents_frequency: Reference frequency = %.3f (MHz)",
              1e-6 * reference_frequency)

    newsc_list = []
    for sc in sc_list:
        newsc = sc.copy()
        x = (frequency - reference_frequency) / reference_frequency
        y = sc.flux
        coeffs = polynomial.polyfit(x, y, nmoment - 1)
        newsc.flux = polynomial.polyval(x, coeffs).T
        newsc_list.append(newsc)
    return newsc_list


def transpose_skycomponents_to_channels(sc_list):
    """A SkyComponent list [source] with flux [nchan, npol] as [chan][source]
    with flux [1, npol].

    :param sc_list: list of SkyComponents
    :return: list over channels of lists of single-channel SkyComponents
    """
    newsc_list = []
    nchan = len(sc_list[0].frequency)
    for chan in range(nchan):
        chan_sc_list = []
        for comp in sc_list:
            newcomp = comp.copy()
            newcomp.frequency = numpy.array([comp.frequency[chan]])
            newcomp.flux = comp.flux[chan, :][numpy.newaxis, :]
            chan_sc_list.append(newcomp)
        newsc_list.append(chan_sc_list)
    return newsc_list


def gather_skycomponents_from_channels(sc_list):
    """Lists [chan][source] of single-frequency SkyComponents as one list
    [source] of multi-frequency SkyComponents.

    :param sc_list: list over channels of lists of SkyComponents
    :return: list of SkyComponents, flux [nchan, npol]
    """
    nsource = len(sc_list[0])
    nchan = len(sc_list)
    newsc_list = []
    for source in range(nsource):
        newcomp = sc_list[0][source].copy()
        flux = numpy.array([sc_list[chan][source].flux[0, :] for chan in range(nchan)])
        frequency = numpy.array([sc_list[chan][source].frequency[0] for chan in range(nchan)])
        newcomp.frequency = frequency
        newcomp.flux = flux
        newsc_list.append(newcomp)
    return newsc_list
