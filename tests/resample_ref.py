"""NUMERICS.md rule 18 restated on the host: what wifirx_channel_sro (wr_channel.hip) computes, value for value -- the
polyphase resampler in NumPy float32 in front of tests/channel_ref.py's rule 17.

Output n of a row reads its input at n + D / 2^40, D = drift0 + dinc n (exact integers): i = n + (D >> 40), mu = D mod 2^40,
table row p = mu >> 33, frac = ((mu >> 9) & 0xFFFFFF) 2^-24, c_k = T[p][k] + frac (T[p+1][k] - T[p][k]),
u[n] = sum_k c_k x[i + k - 15] with plain float32 products per part, from the k = 0 product in ascending k, x = 0 outside
the row.  The table comes from the built library (wifirx_resampler_table)."""
import numpy as np

import channel_ref
from wifirx import capi

F32 = np.float32
N_PHASES, N_TAPS, CENTER = 128, 32, 15
FRAC_BITS = 40
SRO_MAX = 2.0 ** -8
_TABLE = None


def table() -> np.ndarray:
    global _TABLE
    if _TABLE is None:
        _TABLE = capi.resampler_table()
        assert _TABLE.shape == (N_PHASES + 1, N_TAPS) and _TABLE.dtype == F32
    return _TABLE


def drift_inc(sro) -> int:
    """llround((double)sro * 2^40) for the float32 value of sro, in exact integer arithmetic: a float32 is m 2^e, so the
    product is an integer shifted, rounded half away from zero"""
    m, e = np.frexp(np.float64(F32(sro)))
    mi = int(m * 2 ** 53)                 # exact: |m| in [0.5, 1)
    sh = int(e) - 53 + FRAC_BITS
    if sh >= 0:
        return mi << sh
    a = abs(mi)
    k = (a + (1 << (-sh - 1))) >> -sh
    return -k if mi < 0 else k


def locked_sro(cfo, bandwidth=20e6, frequency=5.89e9):
    """epsilon - 1 of a sample clock locked to the carrier: -cfo bw / (2 pi fc), cfo in rad/sample as exp(+j cfo n)"""
    return F32(-float(cfo) * bandwidth / (2 * np.pi * frequency))


def coefficients(D):
    """int64 drifts [n] -> (integer parts D >> 40 [n] int64, float32 taps [n, 32])"""
    D = np.asarray(D, dtype=np.int64)
    T = table()
    mu = D & np.int64((1 << FRAC_BITS) - 1)
    p = (mu >> np.int64(33)).astype(np.intp)
    frac = ((mu >> np.int64(9)) & np.int64(0xFFFFFF)).astype(F32) * F32(2.0 ** -24)
    t0, t1 = T[p], T[p + 1]
    return D >> np.int64(FRAC_BITS), t0 + frac[:, None] * (t1 - t0)


def resample_row(x, dinc=0, drift0=0) -> np.ndarray:
    """one row: complex64 [n] -> the resampled row u, complex64 [n]"""
    x = np.asarray(x, dtype=np.complex64)
    n = x.size
    if n == 0:
        return x.copy()
    assert abs(drift0) + abs(dinc) * n < 1 << 62
    D = np.int64(drift0) + np.int64(dinc) * np.arange(n, dtype=np.int64)
    whole, c = coefficients(D)
    i = np.arange(n, dtype=np.int64) + whole
    xr, xi = x.real.astype(F32), x.imag.astype(F32)
    ur = ui = None
    for k in range(N_TAPS):
        m = i + (k - CENTER)
        ok = (m >= 0) & (m < n)
        mc = np.clip(m, 0, n - 1)
        vr = np.where(ok, xr[mc], F32(0))
        vi = np.where(ok, xi[mc], F32(0))
        pr, pi = c[:, k] * vr, c[:, k] * vi
        ur, ui = (pr, pi) if k == 0 else (ur + pr, ui + pi)
    u = np.empty(n, np.complex64)
    u.real, u.imag = ur, ui
    return u


def channel(x, row_off=None, taps=(1.0,), cfo=None, phase0=0, sro=None, drift0=0, gain=1.0, noise_voltage=0.0, seed=0,
            sample0=0):
    """WifiRx.channel(..., sro=, drift0=) restated: channel_ref.channel with every row resampled first.  sro: scalar or per
    row (taken as float32), None = rule 17 alone."""
    return channel_ref.channel(x, row_off, taps, cfo, phase0, gain, noise_voltage, seed, sample0, sro=sro, drift0=drift0)
