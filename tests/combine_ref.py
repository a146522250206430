"""NUMERICS.md rule 22 in NumPy float32: the critically sampled M-channel synthesis bank of wifirx_combine, in the kernel's
order of operations, and the float64 definition it is measured against.

Channel rows are complex64 [M, n_in]; the wide stream is complex64 [n_in M]; a history is complex64 [M, 23]."""
import numpy as np

import channelizer_ref as zr

TAPS_PER_BRANCH = zr.TAPS_PER_BRANCH
HIST = TAPS_PER_BRANCH - 1
CHANNELS = zr.CHANNELS


def branch_constants(M):
    """c'_r of stacking 1: the complex conjugate of rule 21's float32 constants"""
    return zr.branch_constants(M, conj=True)


def twiddles(M):
    """exp(+j 2 pi t / M), t < M/2: the complex conjugate of rule 21's float32 twiddles"""
    return zr.twiddles(M, conj=True)


def rows(streams, M):
    u = np.ascontiguousarray(np.asarray(streams, dtype=np.complex64))
    assert u.ndim == 2 and u.shape[0] == M
    return u


def history(streams, hist, M):
    """(hist || streams) per channel as complex64 [M, 23 + n_in]; hist None: zeros"""
    u = rows(streams, M)
    h = np.zeros((M, HIST), np.complex64) if hist is None else rows(hist, M)
    assert h.shape == (M, HIST)
    return np.concatenate([h, u], axis=1)


def next_history(streams, hist, M):
    """what hist_out receives: the last 23 samples of (hist || streams) per channel, complex64 [M, 23]"""
    return np.ascontiguousarray(history(streams, hist, M)[:, -HIST:])


def inverse_dft(ur, ui, M):
    """V_r = sum_k u_k exp(+j 2 pi k r / M) down axis 0 of float32 arrays [M, n]: rule 21's radix-2 network with the
    conjugate twiddles"""
    return zr.radix2(ur, ui, M, inverse=True)


def combine(streams, M, s, gains=None, hist=None, m0=0, taps=None):
    """streams: complex64 [M, n_in] -> complex64 [n_in M], the wide stream at M times the rate"""
    assert M in CHANNELS and s in (0, 1)
    h = np.asarray(zr.table(M) if taps is None else taps, dtype=np.float32)
    assert h.shape == (TAPS_PER_BRANCH * M,)
    T = h * np.float32(M)                                     # exact: M is a power of two
    uu = history(streams, hist, M)
    n_in = uu.shape[1] - HIST
    ur, ui = np.ascontiguousarray(uu.real), np.ascontiguousarray(uu.imag)
    if gains is not None:
        g = np.asarray(gains, dtype=np.float32).reshape(M, 1)
        ur, ui = ur * g, ui * g
    vr, vi = inverse_dft(ur, ui, M)                           # [r, 23 + block]
    # branch sums: a[r, m], ascending p from the p = 0 product
    ms = np.arange(n_in, dtype=np.int64)
    ar = ai = None
    for p in range(TAPS_PER_BRANCH):
        t = T[p * M:(p + 1) * M, None]
        tr, ti = t * vr[:, HIST + ms - p], t * vi[:, HIST + ms - p]
        ar, ai = (tr, ti) if p == 0 else (ar + tr, ai + ti)
    # branch constants
    r = np.arange(M)
    if s == 0:
        sign = np.where(r & 1, np.float32(-1), np.float32(1))[:, None]
        xr, xi = ar * sign, ai * sign                         # a sign change
    else:
        cr_, ci_ = branch_constants(M)
        xr, xi = ar.copy(), ai.copy()
        xr[1:], xi[1:] = zr._mul(cr_[1:, None], ci_[1:, None], ar[1:], ai[1:])          # c'_0 = 1 is not multiplied
        neg = ((int(m0) + ms) & 1).astype(bool)
        xr[:, neg], xi[:, neg] = -xr[:, neg], -xi[:, neg]     # the block sign, last
    assert xr.dtype == np.float32 and xi.dtype == np.float32
    out = np.empty((n_in, M), np.complex64)
    out.real, out.imag = xr.T, xi.T
    return out.reshape(-1)


def direct(streams, M, s, taps, gains=None, hist=None, m0=0):
    """the definition in float64, literally: every stream zero-stuffed to M times the rate, convolved with M h, put on its
    carrier exp(j 2 pi f_k n), n the stream's output index, and summed -> complex128 [n_in M]"""
    uu = history(streams, hist, M).astype(np.complex128)
    n_all = uu.shape[1]
    h = np.asarray(taps, dtype=np.float64) * M
    g = np.ones(M) if gains is None else np.asarray(gains, dtype=np.float32).astype(np.float64)
    n = (int(m0) - HIST) * M + np.arange(n_all * M)
    x = np.zeros(n_all * M, np.complex128)
    for k in range(M):
        up = np.zeros(n_all * M, np.complex128)
        up[::M] = uu[k]
        x += g[k] * np.exp(2j * np.pi * zr.centre(k, M, s) * n) * np.convolve(up, h)[:n_all * M]
    return x[HIST * M:]


def term_sum(streams, M, taps, gains=None, hist=None):
    """S[n] = sum_p |M h[pM + r]| sum_k |g_k u_k[m - p]|: the sum of the absolute values of an output's terms, float64"""
    uu = np.abs(history(streams, hist, M).astype(np.complex128))
    g = np.ones(M) if gains is None else np.abs(np.asarray(gains, dtype=np.float32).astype(np.float64))
    tot = (g[:, None] * uu).sum(axis=0)                       # [23 + block]
    h = np.abs(np.asarray(taps, dtype=np.float64)) * M
    n_in = uu.shape[1] - HIST
    ms = np.arange(n_in)
    S = np.zeros((n_in, M))
    for p in range(TAPS_PER_BRANCH):
        S += tot[HIST + ms - p, None] * h[None, p * M:(p + 1) * M]
    return S.reshape(-1)
