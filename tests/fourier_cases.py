"""Cases that tests/golden/make_golden_fourier.py and tests/test_fourier_transforms.py share."""

# w_beam cases: (npixel, field of view, w, cx, cy, remove_shift)
W_BEAM_CASES = {
    "even": (8, 0.3, 57.0, None, None, False),
    "odd": (9, 0.3, 57.0, None, None, False),
    "even_centre": (8, 0.3, -31.5, 3, 4, False),
    "odd_centre": (9, 0.3, -31.5, 4, 3, False),
    "even_shift": (8, 0.3, 57.0, 3, 3, True),
    "odd_shift": (9, 0.3, 57.0, None, None, True),
    "even_corner": (8, 3.0, 7.3, None, None, False),
    "odd_corner": (9, 3.0, 7.3, None, None, False),
}
