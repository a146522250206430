"""NUMERICS.md rule 34 in NumPy float32: the rational resampler of wifirx_arb_resample, in the kernel's order of operations,
the host integers of wifirx_arb_count / wifirx_arb_hist, and the float64 definition the rule is measured against.

Samples are float32 pairs [n, 2] (or the integers of convert_ref's formats, widened by rule 20 first); the output is float32
pairs [n_out, 2].  num / den = fs_in / fs_out is the step in input samples per output sample.

`mutant` names ONE deliberate mistake (MUTANTS); tests/test_arb_ref.py asserts which test catches each."""
import math

import numpy as np

import convert_ref as cr

HALF, PER_UNIT, BETA = 16, 128, 6.5
ENTRIES = 2 * HALF * PER_UNIT + 1
HIST_MAX = 128
MAX_DEN, MAX_NUM, MAX_RATIO = 512, 2048, 4
MUTANTS = ("trunc_div", "frac_div", "gain_on_coef", "descending", "jlo_off")
# the ratios the tests run: up and down through 25, 30.72, 40, 61.44 and 80 MS/s, 1/1, one that is not reduced, and
# 61.44 -> 80 MS/s, whose S = 125 shares no factor with 128 (r then takes every value below S)
RATIOS = ((1, 1), (5, 4), (4, 5), (192, 125), (125, 192), (2, 1), (1, 2), (4, 1), (1, 4), (384, 125), (125, 384), (10, 8), (96, 125))


def prototype(u):
    """h(u) in float64, 0 outside |u| <= 16: the Kaiser-windowed sinc of the rule"""
    u = np.asarray(u, dtype=np.float64)
    w = np.sqrt(np.clip(1.0 - (u / HALF) ** 2, 0.0, None))
    return np.where(np.abs(u) <= HALF, np.sinc(u) * np.i0(BETA * w) / np.i0(BETA), 0.0)


_TABLE = None


def table():
    """H: 4097 float32, h(-16 + q / 128) rounded once; exact 0 at the non-zero integers and exact 1 at 0"""
    global _TABLE
    if _TABLE is None:
        q = np.arange(ENTRIES)
        h = prototype(-HALF + q / PER_UNIT)
        h[q % PER_UNIT == 0] = 0.0
        h[HALF * PER_UNIT] = 1.0
        _TABLE = h.astype(np.float32)
        _TABLE.setflags(write=False)
    return _TABLE


def reduce(num, den):
    """the ratio in lowest terms; ValueError outside the rule's limits"""
    num, den = int(num), int(den)
    if num <= 0 or den <= 0:
        raise ValueError("num and den must be positive")
    g = math.gcd(num, den)
    num, den = num // g, den // g
    if den > MAX_DEN or num > MAX_NUM or num > MAX_RATIO * den or den > MAX_RATIO * num:
        raise ValueError("ratio outside 1 <= den <= 512, 1 <= num <= 2048, 1/4 <= num/den <= 4")
    return num, den


def hist_len(num, den):
    """HL = ceil(32 S / den)"""
    num, den = reduce(num, den)
    S = max(num, den)
    return -((-32 * S) // den)


def m_end(num, den, E):
    """the outputs that the inputs [0, E) make: m < max(0, ceil((E den - 16 S) / num))"""
    num, den = reduce(num, den)
    S = max(num, den)
    return max(0, -((-(int(E) * den - 16 * S)) // num))


def count(num, den, j0, n_in, m0):
    """n_out of a call: m0 .. m_end(j0 + n_in) - 1"""
    return max(0, m_end(num, den, int(j0) + int(n_in)) - int(m0))


def span(num, den, m, mutant=None):
    """(jlo, jhi) of output m as Python integers, floors towards minus infinity"""
    num, den = reduce(num, den)
    S = max(num, den)
    N = int(m) * num
    D = N - 16 * S
    if mutant == "trunc_div" and D < 0:
        jlo = -((-D) // den) + 1                              # C's division: towards zero
    else:
        jlo = D // den + 1
    if mutant == "jlo_off":
        jlo += 1
    return jlo, (N + 16 * S) // den


def _jlo_array(num, den, S, ms, mutant):
    """jlo of every output in ms (int64 array; the products stay below 2^62)"""
    D = ms * num - 16 * S
    if mutant == "trunc_div":
        jlo = np.where(D < 0, -((-D) // den), D // den) + 1
    else:
        jlo = D // den + 1                                    # NumPy's // floors
    return jlo + 1 if mutant == "jlo_off" else jlo


def coefficients(num, den, m):
    """(jlo, c): the float32 coefficients of output m's inputs jlo .. jhi, one output at a time (the rule read literally)"""
    num, den = reduce(num, den)
    S = max(num, den)
    rS = np.float32(1.0) / np.float32(S)
    H = table()
    jlo, jhi = span(num, den, m)
    c = np.empty(jhi - jlo + 1, np.float32)
    for k, j in enumerate(range(jlo, jhi + 1)):
        B = (int(m) * num - j * den + 16 * S) * 128
        assert 0 <= B < 4096 * S
        q, r = divmod(B, S)
        frac = np.float32(r) * rS
        c[k] = H[q] + frac * (H[q + 1] - H[q])
    return jlo, c


def history(x, hist, HL):
    """(hist || x) as float32 pairs; hist = the HL samples in front of x, or None for zeros"""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    h = np.zeros((HL, 2), np.float32) if hist is None else np.asarray(hist, dtype=np.float32).reshape(-1, 2)
    assert len(h) == HL
    return np.concatenate([h, x])


def resample(x, num, den, hist=None, j0=0, m0=0, outputs=None, mutant=None):
    """x: float32 pairs [n_in, 2], in[0] at stream index j0 -> float32 pairs [n_out, 2], the outputs m0 .. m_end - 1 (or the
    stream indices `outputs` among them).  Vectorised over the outputs, a loop over the taps."""
    num, den = reduce(num, den)
    S = max(num, den)
    HL = hist_len(num, den)
    rS = np.float32(1.0) / np.float32(S)
    H = table()
    xx = history(x, hist, HL)                                 # xx[i] is stream sample j0 - HL + i
    n_in = len(xx) - HL
    n_out = count(num, den, j0, n_in, m0)
    ms = (np.arange(n_out, dtype=np.int64) + int(m0)) if outputs is None else np.asarray(outputs, dtype=np.int64)
    if len(ms) == 0:
        return np.zeros((0, 2), np.float32)
    N = ms * num
    jlo = _jlo_array(num, den, S, ms, mutant)
    jhi = (N + 16 * S) // den
    assert int(jlo.min()) >= int(j0) - HL, "the history does not reach"
    assert int(jhi.max()) < int(j0) + n_in
    taps = int((jhi - jlo).max()) + 1
    gain = np.float32(den) / np.float32(S)
    acc_r = acc_i = None
    order = range(taps - 1, -1, -1) if mutant == "descending" else range(taps)
    started = np.zeros(len(ms), bool)
    for k in order:
        j = jlo + k
        live = j <= jhi
        jj = np.where(live, j, jlo)
        B = (N - jj * den + 16 * S) * 128
        B = np.clip(B, 0, 4096 * S - 1)                       # only the jlo_off mutant leaves the range
        q, r = B // S, B % S
        if mutant == "frac_div":
            frac = r.astype(np.float32) / np.float32(S)
        else:
            frac = r.astype(np.float32) * rS
        c = H[q] + frac * (H[q + 1] - H[q])
        if mutant == "gain_on_coef" and num > den:
            c = c * gain
        at = jj - (int(j0) - HL)
        sr = np.where(jj < 0, np.float32(0), xx[at, 0])       # x[j] = 0 in front of the stream
        si = np.where(jj < 0, np.float32(0), xx[at, 1])
        with np.errstate(invalid="ignore", over="ignore"):
            tr, ti = c * sr, c * si
            if acc_r is None:
                acc_r, acc_i = tr.copy(), ti.copy()
            else:
                first = live & ~started
                add = live & started
                acc_r = np.where(first, tr, np.where(add, acc_r + tr, acc_r))
                acc_i = np.where(first, ti, np.where(add, acc_i + ti, acc_i))
        started |= live
    with np.errstate(invalid="ignore", over="ignore"):
        if num > den and mutant != "gain_on_coef":
            acc_r, acc_i = acc_r * gain, acc_i * gain
    assert acc_r.dtype == np.float32 and acc_i.dtype == np.float32
    return np.stack([acc_r, acc_i], axis=1)


def resample_format(q, fmt, scale, num, den, hist=None, j0=0, m0=0, outputs=None):
    """the same on samples of a format: integers [n, 2] are widened by rule 20 (and so is hist), fc32 passes through"""
    if fmt == cr.FC32:
        return resample(q, num, den, hist, j0, m0, outputs)
    return resample(cr.widen(q, scale), num, den, None if hist is None else cr.widen(hist, scale), j0, m0, outputs)


def next_history(x, hist, num, den):
    """what hist_out receives: the last HL samples of (hist || x), in x's own dtype"""
    HL = hist_len(num, den)
    x = np.asarray(x).reshape(-1, 2)
    h = np.zeros((HL, 2), x.dtype) if hist is None else np.asarray(hist, dtype=x.dtype).reshape(-1, 2)
    return np.concatenate([h, x])[-HL:]


def stream(x, num, den, n_out=None, mutant=None):
    """a whole stream from j0 = m0 = 0 on complex samples: complex64 [n_out]; with n_out given, zeros are pushed behind x
    until that many outputs exist (the end-of-stream flush)"""
    x = np.asarray(x, dtype=np.complex64).reshape(-1)
    if n_out is not None:
        x = np.concatenate([x, np.zeros(flush_inputs(num, den, len(x), n_out), np.complex64)])
    y = cr.to_complex(resample(cr.pairs(x), num, den, mutant=mutant))
    return y if n_out is None else y[:n_out]


def flush_inputs(num, den, n_in, n_out):
    """the fewest zeros behind n_in inputs with which m_end reaches n_out"""
    num, den = reduce(num, den)
    S = max(num, den)
    need = ((int(n_out) - 1) * num + 16 * S) // den + 1       # the smallest E with m_end(E) >= n_out, for n_out >= 1
    return max(0, need - int(n_in)) if n_out > 0 else 0


def direct(x, num, den, outputs=None):
    """the definition in float64 from the analytic prototype: y[m] = g sum_j h((m num - j den) / S) x[j], g = den / S for
    num > den and 1 otherwise; x complex from the start of a stream -> complex128 over m < m_end (or `outputs`)"""
    num, den = reduce(num, den)
    S = max(num, den)
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    ms = np.arange(m_end(num, den, len(x)), dtype=np.int64) if outputs is None else np.asarray(outputs, dtype=np.int64)
    j = np.arange(len(x), dtype=np.int64)
    y = np.empty(len(ms), np.complex128)
    for a in range(0, len(ms), 256):
        u = (ms[a:a + 256, None] * num - j[None, :] * den) / float(S)
        y[a:a + 256] = prototype(u) @ x
    return y * (den / float(S) if num > den else 1.0)


def coefficient_sum(num, den):
    """max over the den phases of sum_j |c|, float64 from the float32 table (before the gain)"""
    num, den = reduce(num, den)
    S = max(num, den)
    H = table().astype(np.float64)
    worst = 0.0
    for ph in range(den):
        B = np.arange(ph * 128, 4096 * S, den * 128)
        q, r = B // S, B % S
        worst = max(worst, float(np.abs(H[q] + r / float(S) * (H[q + 1] - H[q])).sum()))
    return worst


def error_bound(num, den, max_component):
    """the rule's bound on |restatement - direct()| per component: T taps, each coefficient off h(u) by at most the linear
    interpolation's max|h''| / (8 * 128^2) with max|h''| <= 3.4, plus 5 roundings of 2^-24 (the table entry, the subtract,
    frac, its product, the add); each product and each add one rounding of a value below sum|c| max|x|; two for the gain"""
    num, den = reduce(num, den)
    S = max(num, den)
    T = 32 * S // den + 1
    g = den / float(S) if num > den else 1.0
    e_coef = 3.4 / (8 * PER_UNIT ** 2) + 5 * 2.0 ** -24
    return g * max_component * (T * e_coef + (2 * T + 2) * 2.0 ** -24 * coefficient_sum(num, den))
