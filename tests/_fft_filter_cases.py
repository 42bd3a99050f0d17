"""Cases of the FFT-filter fixture (tests/golden/fft_filter.npz), shared by its generator (which builds the transfer
functions with the reference's own window functions) and the tests (which build them with kikuchipy_amd.filters).

A case is (function_domain, shift, build) with `build(shape, f)` -> the transfer function or kernel for patterns of
`shape`; `f` supplies `lowpass(shape, cutoff, width)`, `highpass(shape, cutoff, width)`, `hann(n)` and
`window(name, shape, **kw)`.  The synthetic inputs are tests/_iq_inputs.py's."""

import numpy as np


def _gauss(n, std):
    x = np.arange(n) - (n - 1) / 2.0
    return np.exp(-0.5 * (x / std) ** 2)


def _nonsym(shape):
    k, l = np.mgrid[: shape[0], : shape[1]]
    return ((7 * k + 3 * l) % 11 + 1 + 0.25 * k) / 11.0


def _complex(shape):
    k, l = np.mgrid[: shape[0], : shape[1]]
    return np.cos(0.3 * k + 0.2 * l) + 1j * np.sin(0.11 * k - 0.07 * l) + 0.5


CASES = {
    # frequency domain
    "lowhigh": ("frequency", True, lambda s, f: f.lowpass(s, 22, 10) * f.highpass(s, 1, 0.5)),  # the tutorial's
    "highpass": ("frequency", False, lambda s, f: f.highpass(s, 2, 1)),
    "hann": ("frequency", True, lambda s, f: np.outer(f.hann(s[0]), f.hann(s[1]))),
    "gauss": ("frequency", True, lambda s, f: np.outer(_gauss(s[0], max(1.0, s[0] / 6)), _gauss(s[1], max(1.0, s[1] / 6)))),
    "nonsym": ("frequency", False, lambda s, f: _nonsym(s)),
    "complex": ("frequency", True, lambda s, f: _complex(s)),
    # spatial domain
    "sobel": ("spatial", False, lambda s, f: np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]], dtype=np.float64)),
    "gauss5": ("spatial", False, lambda s, f: np.outer(_gauss(5, 1.0), _gauss(5, 1.0))),
    "circ7": ("spatial", False, lambda s, f: np.asarray(f.window("circular", (7, 7)), dtype=np.float64)),
    "k3x7": ("spatial", False, lambda s, f: np.arange(21).reshape(3, 7) % 5 - 2.0),
    "even4": ("spatial", False, lambda s, f: ((np.arange(16).reshape(4, 4) * 7) % 9) / 9.0),
    "big": ("spatial", False, lambda s, f: np.outer(np.linspace(0.2, 1, s[0] + 3), np.linspace(1, 0.3, s[1] + 2))),
}
NAMES = list(CASES)
NI_CORRECTED_CASES = ["lowhigh", "hann", "sobel", "gauss5"]
N_STORED = 2  # synthetic stacks: the first two patterns are stored


def synthetic_case(shape_index, dtype_index):
    """The one case stored for a synthetic (shape, dtype): rotated so that every case meets several shapes."""
    return NAMES[(3 * shape_index + 5 * dtype_index) % len(NAMES)]


class OurFunctions:
    """`f` of the cases, from kikuchipy_amd.filters."""

    def __init__(self):
        from kikuchipy_amd import filters

        self.lowpass = filters.lowpass_fft_filter
        self.highpass = filters.highpass_fft_filter
        self.hann = filters.modified_hann
        self.window = filters.Window
