"""NUMERICS.md rule 36 in NumPy float32: the band survey -- windowed-FFT power rows of a stream, the fold of rows, the band
powers of rows and the bins of a band -- value for value as wr_spectrum.hip computes them, with the float64 definition next to
it.  The tables are the library's own (wifirx_spectrum_table).  Samples are float32 pairs [n, 2]."""
import math

import numpy as np

import convert_ref as cr
from wifirx import capi

N_FFT = (64, 256, 1024, 4096)
ENTRIES = 4096
RECT, HANN, BLACKMAN_HARRIS = 0, 1, 2
SUM, MAX = 0, 1
MAX_BANDS, MAX_HOP = 16, 1 << 20
BH = (0.35875, 0.48829, 0.14128, 0.01168)
U = 2.0 ** -24                                            # the relative error of one float32 rounding

MUTANTS = ("window_index_off_by_one", "twiddle_stride", "no_digit_reversal", "no_centre_shift", "hop_off_by_one", "max_for_sum",
           "norm_per_segment")

_tables = None


def tables():
    """(hann [4096], blackman_harris [4096], twiddle [4096, 2]) float32, read once through the C ABI"""
    global _tables
    if _tables is None:
        _tables = capi.spectrum_table()
    return _tables


def window_table(window):
    return None if window == RECT else tables()[0 if window == HANN else 1]


def count(n_fft, hop, avg, n_in):
    """(n_rows, consumed): S = (n_in - N) // hop + 1 segments (0 below N), n_rows = S // avg, consumed = n_rows avg hop"""
    S = (n_in - n_fft) // hop + 1 if n_in >= n_fft else 0
    rows = S // avg
    return rows, rows * avg * hop


def digit_reverse(n_fft):
    """rev[i]: the base-4 digits of i in reverse order"""
    D = int(round(math.log(n_fft, 4)))
    i = np.arange(n_fft)
    k = np.zeros(n_fft, np.int64)
    for _ in range(D):
        k = (k << 2) | (i & 3)
        i = i >> 2
    return k


def fft_power(re, im, mutant=None):
    """[S, N] float32 parts of the windowed segments -> [S, N] float32 powers, bin i = frequency (i - N/2) / N"""
    S, N = re.shape
    T = tables()[2]
    re, im = re.copy(), im.copy()
    L = N // 4
    with np.errstate(invalid="ignore", over="ignore"):
        while L >= 1:
            r, m = re.reshape(S, -1, 4, L), im.reshape(S, -1, 4, L)
            ar, br, cr_, dr = r[:, :, 0], r[:, :, 1], r[:, :, 2], r[:, :, 3]
            ai, bi, ci, di = m[:, :, 0], m[:, :, 1], m[:, :, 2], m[:, :, 3]
            t0r, t0i, t1r, t1i = ar + cr_, ai + ci, ar - cr_, ai - ci
            t2r, t2i, t3r, t3i = br + dr, bi + di, br - dr, bi - di
            yr = [t0r + t2r, t1r + t3i, t0r - t2r, t1r - t3i]
            yi = [t0i + t2i, t1i - t3r, t0i - t2i, t1i + t3r]
            n = np.arange(L)
            stride = ENTRIES // 4 // L
            if mutant == "twiddle_stride":
                stride = ENTRIES // N
            new_r, new_i = np.empty_like(r), np.empty_like(m)
            new_r[:, :, 0], new_i[:, :, 0] = yr[0], yi[0]
            for q in (1, 2, 3):
                c = T[(q * n * stride) % ENTRIES]
                pr = c[:, 0] * yr[q] - c[:, 1] * yi[q]
                pi = c[:, 0] * yi[q] + c[:, 1] * yr[q]
                new_r[:, :, q] = np.where(n == 0, yr[q], pr)          # exponent 0 is not multiplied at all
                new_i[:, :, q] = np.where(n == 0, yi[q], pi)
            re, im = new_r.reshape(S, N), new_i.reshape(S, N)
            assert re.dtype == np.float32
            L //= 4
        p = re * re + im * im
    if mutant != "no_digit_reversal":
        p = p[:, digit_reverse(N)]
    if mutant != "no_centre_shift":
        p = np.roll(p, N // 2, axis=1)
    return p


def fold_values(a, p, mode):
    """one step of the fold, elementwise: SUM a + p; MAX (p > a or p is NaN) ? p : a"""
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == MAX:
            return np.where((p > a) | (p != p), p, a)
        return a + p


def spectrum(x, n_fft, hop, avg, window=BLACKMAN_HARRIS, mode=SUM, norm=1.0, mutant=None):
    """x float32 [n, 2] -> float32 [n_rows, n_fft]"""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    rows, _ = count(n_fft, hop, avg, len(x))
    out = np.zeros((rows, n_fft), np.float32)
    if rows == 0:
        return out
    step = hop + 1 if mutant == "hop_off_by_one" else hop
    starts = np.arange(rows * avg) * step
    starts = np.minimum(starts, len(x) - n_fft)               # only the mutant's starts can leave the stream
    seg = x[starts[:, None] + np.arange(n_fft)[None, :]]      # [S, N, 2]
    re, im = seg[:, :, 0], seg[:, :, 1]
    w = window_table(window)
    if w is not None:
        idx = np.arange(n_fft) * (ENTRIES // n_fft)
        if mutant == "window_index_off_by_one":
            idx = (idx + ENTRIES // n_fft) % ENTRIES
        with np.errstate(invalid="ignore"):
            re, im = w[idx] * re, w[idx] * im
    p = fft_power(np.ascontiguousarray(re), np.ascontiguousarray(im), mutant).reshape(rows, avg, n_fft)
    nf = np.float32(norm)
    if mutant == "max_for_sum":
        mode = MAX if mode == SUM else SUM
    with np.errstate(invalid="ignore", over="ignore"):
        if mutant == "norm_per_segment" and mode == MAX:
            p = p * nf
        a = p[:, 0]
        for s in range(1, avg):
            a = fold_values(a, p[:, s], mode)
        if not (mutant == "norm_per_segment" and mode == MAX):
            a = a * nf
    assert a.dtype == np.float32
    return a


def spectrum_format(q, fmt, scale, n_fft, hop, avg, window=BLACKMAN_HARRIS, mode=SUM, norm=1.0):
    """the same on samples of a format: integers [n, 2] are widened by rule 20 first, fc32 passes through"""
    return spectrum(q if fmt == cr.FC32 else cr.widen(q, scale), n_fft, hop, avg, window, mode, norm)


def fold(rows, group, mode):
    """float32 [n_rows, N] -> [n_rows // group, N]: the ascending fold of each group of rows"""
    rows = np.asarray(rows, dtype=np.float32)
    made = rows.shape[0] // group
    r = rows[:made * group].reshape(made, group, rows.shape[1])
    a = r[:, 0]
    for g in range(1, group):
        a = fold_values(a, r[:, g], mode)
    return np.ascontiguousarray(a)


def bands(rows, edges):
    """float32 [n_rows, N], edges [(lo, hi), ..] -> float32 [n_rows, n_bands]: lane l adds bins lo + l, lo + l + 64, .. below hi
    from its first bin's value (+0 without one), then lane xor 1, 2, 4, 8, 16, 32"""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.zeros((rows.shape[0], len(edges)), np.float32)
    lane = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, (lo, hi) in enumerate(edges):
            v = np.zeros((rows.shape[0], 64), np.float32)
            t = 0
            while lo + 64 * t < hi:
                i = lo + lane + 64 * t
                ok = i < hi
                val = rows[:, np.minimum(i, hi - 1)]
                v = np.where(ok[None, :], val if t == 0 else v + val, v)
                t += 1
            for m in (1, 2, 4, 8, 16, 32):
                v = v + v[:, lane ^ m]
            assert v.dtype == np.float32
            out[:, b] = v[:, 0]
    return out


def band(offset_hz, width_hz, sample_rate, n_fft):
    """(lo, hi) of wifirx_spectrum_band in float64, or None where it answers WIFIRX_ERANGE"""
    a = math.ceil((offset_hz - width_hz / 2) * n_fft / sample_rate)
    b = math.ceil((offset_hz + width_hz / 2) * n_fft / sample_rate)
    half = n_fft // 2
    if a < -half or b > half or a >= b:
        return None
    return a + half, b + half


def window64(window, n_fft):
    """the window from its formula in float64 (periodic forms)"""
    f = 2 * np.pi * np.arange(n_fft) / n_fft
    if window == RECT:
        return np.ones(n_fft)
    if window == HANN:
        return 0.5 - 0.5 * np.cos(f)
    return BH[0] - BH[1] * np.cos(f) + BH[2] * np.cos(2 * f) - BH[3] * np.cos(3 * f)


def definition(x, n_fft, hop, avg, window=BLACKMAN_HARRIS, mode=SUM, norm=1.0):
    """the definition in float64: np.fft.fft of the windowed segments, fftshift, |.|^2, the fold, times norm.  x float32
    [n, 2] (the widened samples) -> float64 [n_rows, n_fft]"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    z = x[:, 0] + 1j * x[:, 1]
    rows, _ = count(n_fft, hop, avg, len(z))
    starts = np.arange(rows * avg) * hop
    seg = z[starts[:, None] + np.arange(n_fft)[None, :]] * window64(window, n_fft)[None, :]
    p = np.abs(np.fft.fftshift(np.fft.fft(seg, axis=1), axes=1)) ** 2
    p = p.reshape(rows, avg, n_fft)
    return (p.max(axis=1) if mode == MAX else p.sum(axis=1)) * float(np.float32(norm))


def error_bound(n_fft, avg):
    """the rule's bound on |restatement - definition| per bin, relative to the row's mean power, for |norm| = 1.
    Norm-wise over a segment, to first order in u = 2^-24: the window costs 1.5 u (the table's rounding u / 2, the product u);
    a stage's butterfly 4 u (each output is three rounded complex adds of values below |a| + |b| + |c| + |d| <= 2 |(a, b, c, d)|,
    and the stage doubles the norm), its twiddle (2 + sqrt 2) u (the table's rounding u, two products and a sum
    (1 + sqrt 2) u); the stages are twice unitary, so earlier errors keep their relative size:
    e_X = (1.5 + (6 + sqrt 2) log4 N) u.  A bin's error is at most the whole vector's, e_X |X|, and |X_k| <= |X|, |X|^2 = N mean:
    the power is off by (2 e_X + e_X^2) N mean, its own product-sum by 2 u N mean, each of the avg - 1 adds of the fold and the
    multiply by norm by u N mean (a row's value is at most N times the row's mean; the MAX fold adds nothing)."""
    D = round(math.log(n_fft, 4))
    e_x = (1.5 + (6 + math.sqrt(2)) * D) * U
    return n_fft * (2 * e_x + e_x * e_x + (2 + avg) * U)
