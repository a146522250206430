"""NUMERICS.md rule 21 in NumPy float32: the critically sampled M-channel analysis bank of wifirx_channelize, in the
kernel's order of operations, and the float64 helpers the tests and examples/make_iq_file.py share.

Samples are float32 pairs [n, 2] (or the integers of convert_ref's formats, widened by rule 20 first); channel rows are
complex64 [M, n_out]."""
import numpy as np

import convert_ref as cr

TAPS_PER_BRANCH = 24
CHANNELS = (2, 4, 8)


def table(M):
    """the float32 prototype, 24 M taps, as the built library hands it out"""
    from wifirx import capi
    return capi.channelizer_table(M)


def centre(k, M, s):
    """f_k in cycles per input sample"""
    return (k + s / 2.0 - M / 2.0) / M


def _snap32(z):
    z = np.asarray(z, dtype=np.complex128)
    re, im = z.real.copy(), z.imag.copy()
    re[np.abs(re) < 1e-15] = 0.0
    im[np.abs(im) < 1e-15] = 0.0
    return re.astype(np.float32), im.astype(np.float32)


def branch_constants(M, conj=False):
    """c_q of stacking 1, float32 (re, im), rounded once from float64; conj: rule 22's, the imaginary part's sign flipped"""
    q = np.arange(M)
    re, im = _snap32((-1.0) ** q * np.exp(-1j * np.pi * q / M))
    return re, -im if conj else im


def twiddles(M, conj=False):
    """exp(-j 2 pi t / M), t < M/2, float32 (re, im), rounded once from float64; conj: the imaginary part's sign flipped"""
    re, im = _snap32(np.exp(-2j * np.pi * np.arange(M // 2) / M))
    return re, -im if conj else im


def _mul(ar, ai, br, bi):
    """rule 17's plain complex product on float32 arrays"""
    return ar * br - ai * bi, ar * bi + ai * br


def _bitrev(j, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (j & 1)
        j >>= 1
    return r


def radix2(xr, xi, M, inverse=False):
    """the M-point DFT (inverse: sum_k x_k exp(+j 2 pi k r / M), the conjugate twiddles) down axis 0 of float32 arrays
    [M, n]: radix 2, decimation in time on the bit-reversed input; W = 1 is not multiplied, W = -+j is a swap and a sign"""
    bits = M.bit_length() - 1
    order = [_bitrev(j, bits) for j in range(M)]
    ar, ai = np.ascontiguousarray(xr[order]), np.ascontiguousarray(xi[order])
    tw_r, tw_i = twiddles(M, conj=inverse)
    length = 2
    while length <= M:                                        # wr_bank.h: for (len = 2; len <= M; len *= 2)
        half = length // 2
        for base in range(0, M, length):
            for t in range(half):
                i0, i1 = base + t, base + t + half
                e = t * (M // length)
                br, bi = ar[i1].copy(), ai[i1].copy()
                if e == 0:
                    tr, ti = br, bi
                elif 4 * e == M:
                    tr, ti = (-bi, br) if inverse else (bi, -br)
                else:
                    tr, ti = _mul(tw_r[e], tw_i[e], br, bi)
                ar[i0], ar[i1] = ar[i0] + tr, ar[i0] - tr
                ai[i0], ai[i1] = ai[i0] + ti, ai[i0] - ti
        length *= 2
    return ar, ai


def history(x, hist, M):
    """(hist || x) as float32 pairs, hist = the 23 M samples in front of x or None for zeros"""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    h = np.zeros((23 * M, 2), np.float32) if hist is None else np.asarray(hist, dtype=np.float32).reshape(-1, 2)
    assert len(h) == 23 * M
    return np.concatenate([h, x])


def analyse(x, M, s, hist=None, m0=0, taps=None, outputs=None):
    """x: float32 pairs [n_out M, 2] -> complex64 [M, n_out] (or [M, len(outputs)] for the output indices `outputs`)"""
    assert M in CHANNELS and s in (0, 1)
    h = np.asarray(table(M) if taps is None else taps, dtype=np.float32)
    assert h.shape == (TAPS_PER_BRANCH * M,)
    xx = history(x, hist, M)
    n_out = (len(xx) - 23 * M) // M
    ms = np.arange(n_out, dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64)
    q = np.arange(M, dtype=np.int64)
    # branch sums: v[m, q], ascending p from the p = 0 product
    vr = vi = None
    for p in range(TAPS_PER_BRANCH):
        g = h[p * M + M - 1 - q]
        if s and (p & 1):
            g = -g
        at = (23 + ms[:, None] - p) * M + q[None, :]
        tr, ti = g[None, :] * xx[at, 0], g[None, :] * xx[at, 1]
        vr, vi = (tr, ti) if p == 0 else (vr + tr, vi + ti)
    # branch constants
    if s == 0:
        sign = np.where(q & 1, np.float32(-1), np.float32(1))[None, :]
        wr_, wi_ = vr * sign, vi * sign                       # a sign change
    else:
        cr_, ci_ = branch_constants(M)
        wr_, wi_ = vr.copy(), vi.copy()
        wr_[:, 1:], wi_[:, 1:] = _mul(cr_[None, 1:], ci_[None, 1:], vr[:, 1:], vi[:, 1:])     # c_0 = 1 is not multiplied
    ar, ai = radix2(wr_.T, wi_.T, M)                          # [k, m]
    if s:
        neg = ((int(m0) + ms) & 1).astype(bool)
        ar[:, neg], ai[:, neg] = -ar[:, neg], -ai[:, neg]
    assert ar.dtype == np.float32 and ai.dtype == np.float32
    out = np.empty((M, len(ms)), np.complex64)
    out.real, out.imag = ar, ai
    return out


def analyse_format(q, fmt, scale, M, s, hist=None, m0=0, outputs=None):
    """the same on samples of a format: integers [n, 2] are widened by rule 20 (and so is hist), fc32 passes through"""
    if fmt == cr.FC32:
        return analyse(q, M, s, hist, m0, outputs=outputs)
    return analyse(cr.widen(q, scale), M, s, None if hist is None else cr.widen(hist, scale), m0, outputs=outputs)


def next_history(x, hist, M):
    """what hist_out receives: the last 23 M samples of (hist || x), in x's own dtype"""
    x = np.asarray(x).reshape(-1, 2)
    h = np.zeros((23 * M, 2), x.dtype) if hist is None else np.asarray(hist, dtype=x.dtype).reshape(-1, 2)
    return np.concatenate([h, x])[-23 * M:]


def direct(x, M, s, taps):
    """the definition in float64: z_k = x exp(-j 2 pi f_k n), convolve with h, take every M-th output from n = M - 1.
    x complex [n_out M] from the start of a stream -> complex128 [M, n_out]"""
    x = np.asarray(x, dtype=np.complex128)
    n = np.arange(len(x))
    h = np.asarray(taps, dtype=np.float64)
    return np.stack([np.convolve(x * np.exp(-2j * np.pi * centre(k, M, s) * n), h)[M - 1:len(x):M] for k in range(M)])


def synthesise(streams, M, s, gains=None):
    """the host synthesis of a wideband capture, the examples' own (txgen.synthesise_wideband): M complex streams at fs ->
    complex128 [n M] at M fs, channel k at f_k"""
    from wifirx import txgen
    return txgen.synthesise_wideband(streams, M, s, gains)
