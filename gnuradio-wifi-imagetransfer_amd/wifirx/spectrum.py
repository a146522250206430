"""Host side of the band survey (wifirx_spectrum, NUMERICS.md rule 36): the scale factors that turn the device's power rows
into power per bin or a power spectral density, decibels, and the decision which candidate channels of a capture are busy.
Everything here is float64 on the host and not under the rule; the rows and the band powers come from the device
(``capi.WifiRx.spectrum``, ``spectrum_bands``; block ``spectrum_probe``)."""
from __future__ import annotations

import numpy as np

BLACKMAN_HARRIS = (0.35875, 0.48829, 0.14128, 0.01168)


def window(name, n_fft) -> np.ndarray:
    """the periodic (DFT-even) window of n_fft points in float64: "rect", "hann" or "blackman_harris" (4 terms)"""
    f = 2 * np.pi * np.arange(int(n_fft)) / int(n_fft)
    if name == "rect":
        return np.ones(int(n_fft))
    if name == "hann":
        return 0.5 - 0.5 * np.cos(f)
    if name == "blackman_harris":
        a = BLACKMAN_HARRIS
        return a[0] - a[1] * np.cos(f) + a[2] * np.cos(2 * f) - a[3] * np.cos(3 * f)
    raise ValueError("window must be 'rect', 'hann' or 'blackman_harris'")


def norm(n_fft, window_name="blackman_harris", avg=1, sample_rate=None) -> float:
    """The ``norm`` argument of wifirx_spectrum for a SUM row of ``avg`` segments.  sample_rate None: power per bin, a tone of
    amplitude A reads A^2 in its bin, 1 / (avg (sum w)^2).  With sample_rate: a power spectral density per Hz (Welch's),
    1 / (avg sample_rate sum w^2), whose sum over the bins times sample_rate / n_fft is the stream's mean power.  For MAX rows
    pass avg = 1."""
    w = window(window_name, n_fft)
    if sample_rate is None:
        return 1.0 / (float(avg) * float(w.sum()) ** 2)
    return 1.0 / (float(avg) * float(sample_rate) * float((w * w).sum()))


def to_db(p, floor=1e-30) -> np.ndarray:
    """10 log10 of powers, values below ``floor`` (zeros) taken as ``floor``"""
    return 10.0 * np.log10(np.maximum(np.asarray(p, dtype=np.float64), floor))


def busy_channels(band_rows, margin_db=10.0) -> list:
    """band_rows [n_rows, n_bands]: the power of each candidate band (of one width) per row, as wifirx_spectrum_bands gives
    it.  The floor of a band is its smallest row; a band is busy when its largest row stands ``margin_db`` above the lowest
    floor of all bands.  Returns the indices of the busy bands, ascending."""
    r = np.asarray(band_rows, dtype=np.float64)
    if r.ndim != 2 or r.shape[0] == 0:
        return []
    floor = to_db(r.min(axis=0)).min()
    peak = to_db(r.max(axis=0))
    return [int(k) for k in np.nonzero(peak >= floor + float(margin_db))[0]]
