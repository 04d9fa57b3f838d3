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

``find_skycomponents_frequency_taylor_terms`` (:83-153) is left out: it needs
``find_skycomponents``, which segments the image with photutils, and that
package is not available to this project.
"""

import logging

import numpy
from numpy.polynomial import polynomial

__all__ = ["calculate_skycomponent_list_taylor_terms",
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
