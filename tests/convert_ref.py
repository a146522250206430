"""NUMERICS.md rule 20 in NumPy: the sample formats sc16 / sc8, widened to float32 and quantised from it.

Samples are arrays of shape [n, 2] (I, Q), int16 or int8 for the integer formats, float32 for the values (a complex64 array
viewed as float32 pairs); the arithmetic is per component, so any shape works."""
import numpy as np

FC32, SC16, SC8 = 0, 1, 2                       # WIFIRX_IQ_*
DTYPE = {SC16: np.int16, SC8: np.int8}
MAX_BITS = {SC16: 16, SC8: 8}
SCALE = {SC16: np.float32(2.0 ** -15), SC8: np.float32(2.0 ** -7)}


def widen(q, scale):
    """(float)q * scale: one float32 multiply of the exactly converted integer"""
    return np.asarray(q).astype(np.float32) * np.float32(scale)


def quantise(x, scale, fmt, bits=None):
    """x float32 (any shape) -> (integers of the format's dtype, number of clipped components).  t = x * scale in float32,
    r = rint(t) (ties to even), clamp to [-2^(bits-1), 2^(bits-1) - 1]; NaN gives 0; clipped = NaN or r outside the range."""
    bits = MAX_BITS[fmt] if bits is None else bits
    assert 2 <= bits <= MAX_BITS[fmt]
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * np.float32(scale)
        assert t.dtype == np.float32
        r = np.rint(t)
    lo, hi = np.float32(-(2 ** (bits - 1))), np.float32(2 ** (bits - 1) - 1)
    nan = np.isnan(t)
    clipped = nan | (r < lo) | (r > hi)
    q = np.where(nan, np.float32(0), np.clip(r, lo, hi))
    return q.astype(np.int32).astype(DTYPE[fmt]), int(np.count_nonzero(clipped))


def pairs(x):
    """complex64 [n] -> float32 [n, 2]"""
    return np.ascontiguousarray(x, dtype=np.complex64).reshape(-1).view(np.float32).reshape(-1, 2)


def to_complex(v):
    """float32 [n, 2] -> complex64 [n]"""
    return np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 2).view(np.complex64).reshape(-1)


def full_scale(x, backoff_db, fmt, bits=None):
    """The quantiser scale that puts full scale (2^(bits-1)) `backoff_db` dB above the RMS of the complex samples x --
    per component, the RMS of a component being |x|_rms / sqrt(2) -- as a float32"""
    bits = MAX_BITS[fmt] if bits is None else bits
    x = np.asarray(x, dtype=np.complex64).reshape(-1)
    rms = np.sqrt(np.mean(np.abs(x.astype(np.complex128)) ** 2) / 2.0)
    return np.float32(2.0 ** (bits - 1) / (rms * 10.0 ** (backoff_db / 20.0)))
