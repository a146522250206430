"""Frame synchronisation restated: the 384-sample coarse derotation (NUMERICS.md rule 8, the sentence on the samples that
feed the LTS search), the two-stage LTS search (rule 6), sync_long's pair search and the fine CFO (SURVEY.md App. A.3,
products by rule 2) in float32 NumPy, and the same search by its float64 definition.

Written from those texts.  Imports nothing of the product or the oracle (tests/test_lts_rows.py checks that); the
float32 fused multiply-add is detect_ref.fma32; the elementary functions (`sincos`, `atan2`: rule 1) are arguments.
The taps are formed here from the LTS's float64 formula; tests/test_lts_rows.py compares them with include/wifirx_tables.h."""
import numpy as np

from detect_ref import fma32

SYNC = 320                  # sync_long(sync_length): lags searched
WIN = 384                   # copied samples that feed the search
MAX_SAMPLES = 540 * 80
F_DETECTED, F_SYNC, F_TRUNCATED = 0x01, 0x02, 0x80
f32 = np.float32

LTS_M26_26 = [1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1, 1, 1, 1, 0,
              1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, 1, 1]

# switches of the reference mutants (tests/test_lts_rows.py): every one off is the rule
MUTANTS = ("stage1_tie_high", "top4_tie_high", "shortcut_always", "shortcut_never", "no_63_65", "last_pair_wins",
           "nan_is_peak", "clamp_128_wrap", "nan_to_127", "zero_383_before_max", "divide_by_64", "wave_min_is_max",
           "lane_last_slot")


def lts64():
    """the 64-sample LTS in float64: inverse DFT of L(-26..26), scale 1 / sqrt(52); parts below 1e-12 are +0"""
    n = np.arange(64)
    x = np.zeros(64, np.complex128)
    for k, v in zip(range(-26, 27), LTS_M26_26):
        x += v * np.exp(2j * np.pi * k * n / 64.0)
    x /= np.sqrt(52.0)
    re = np.where(np.abs(x.real) < 1e-12, 0.0, x.real)
    im = np.where(np.abs(x.imag) < 1e-12, 0.0, x.imag)
    return re + 1j * im


def taps():
    """(float32 [64, 2] taps rounded once from float64, int64 [64, 2] = rint(64 l) of the float64 values)"""
    l = lts64()
    t = np.stack([l.real, l.imag], axis=1)
    return t.astype(np.float32), np.rint(64.0 * t).astype(np.int64)


def cmul(xr, xi, c, s):
    """rule 2, first form: x (c + j s)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return fma32(-xi, s, xr * c), fma32(xi, c, xr * s)


def window(slot, t):
    """x[t - 16 + m], m = 0..383, as float32 (re, im); +0 outside the slot"""
    slot = np.ascontiguousarray(slot, dtype=np.complex64).reshape(-1)
    xr, xi = np.zeros(WIN, np.float32), np.zeros(WIN, np.float32)
    m = np.arange(WIN)
    ok = (t - 16 + m >= 0) & (t - 16 + m < slot.size)
    xr[ok], xi[ok] = slot.real[t - 16 + m[ok]], slot.imag[t - 16 + m[ok]]
    return xr, xi


def derotate(xr, xi, cfo_c, sincos):
    """y[64 p + l] = x[64 p + l] w_l w64^p: w_l = exp(-j float(cfo_c l)) by sincos of the float32 angle, carried p times
    by w64 = exp(-j float(cfo_c 64)), each step and the product with the sample one rule-2 product"""
    neg = -f32(cfo_c)
    s64, c64 = sincos(np.array([neg * f32(64)], np.float32))
    sl, cl = sincos((neg * np.arange(64).astype(np.float32)).astype(np.float32))
    wr, wi = cl.copy(), sl.copy()
    yr, yi = np.zeros(WIN, np.float32), np.zeros(WIN, np.float32)
    for p in range(WIN // 64):
        if p:
            wr, wi = cmul(wr, wi, c64[0], s64[0])
        yr[64 * p:64 * p + 64], yi[64 * p:64 * p + 64] = cmul(xr[64 * p:64 * p + 64], xi[64 * p:64 * p + 64], wr, wi)
    return yr, yi


def quantise(yr, yi, mut=()):
    """stage 1's 8-bit image: (E, scale, q int64 [768] interleaved re / im, r float32 [768] the rint values before the clamp)"""
    A = np.stack([yr, yi], axis=1).reshape(-1).astype(np.float32)
    bits = A.view(np.uint32)
    ex = ((bits >> 23) & 0xff).astype(np.int64)
    if "zero_383_before_max" in mut:
        ex = ex[:2 * (WIN - 1)]
    E = int(ex.max())
    sfield = min(260 - E, 254)
    scale = np.array([sfield << 23], np.uint32).view(np.float32)[0]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        r = np.rint(A * scale).astype(np.float32)
    lim = 128 if "clamp_128_wrap" in mut else 127
    q = np.where(np.isnan(r), 127 if "nan_to_127" in mut else 0, np.clip(np.nan_to_num(r, nan=0.0, posinf=1e9, neginf=-1e9), -lim, lim)).astype(np.int64)
    if "clamp_128_wrap" in mut:
        q = q.astype(np.int8).astype(np.int64)          # +128 wraps to -128
    return E, scale, q, r


def int_magnitudes(q):
    """|conj(lq) yq|^2 of the 320 lags: exact integer sums, fma(im, im, re re) on the exactly converted floats"""
    lq = taps()[1]
    qr, qi = q[0::2], q[1::2]
    wr = np.lib.stride_tricks.sliding_window_view(qr, 64)[:SYNC]
    wi = np.lib.stride_tricks.sliding_window_view(qi, 64)[:SYNC]
    cr = wr @ lq[:, 0] + wi @ lq[:, 1]
    ci = wi @ lq[:, 0] - wr @ lq[:, 1]
    assert max(np.abs(cr).max(), np.abs(ci).max()) < 2 ** 24
    fr, fi = cr.astype(np.float32), ci.astype(np.float32)
    return fma32(fi, fi, fr * fr), cr, ci


def lane_of(lag):
    """the kernel's layout of stage 1: lane 16 q + col holds lags 8 col + 2 q + 128 (s >> 1) + (s & 1), s = 0..5"""
    r = lag % 128
    return 16 * ((r % 8) // 2) + r // 8


def candidates(mag1, mut=()):
    """(shortcut taken, candidate lags): the largest first, lowest lag first among equals; two when they are 64 apart and
    the third value is below 0.875f times the second (one float32 product), else eight"""
    cand = []
    hi = "stage1_tie_high" in mut
    for r in range(8):
        m = mag1.copy()
        m[cand] = -1
        tied = np.flatnonzero(m == m.max())
        best = int(tied[-1 if hi else 0])
        if "lane_last_slot" in mut and len({lane_of(int(i)) for i in tied}) == 1:
            best = int(tied[-1])            # the kernel's single-lane branch taking the LAST slot of the lane that matches
        if "wave_min_is_max" in mut:        # the lowest tied lag of every lane of the kernel's layout, then the HIGHEST of those
            best = max(min(int(i) for i in tied if lane_of(int(i)) == ln) for ln in {lane_of(int(i)) for i in tied})
        if r == 2 and abs(cand[0] - cand[1]) == 64 and "shortcut_never" not in mut:
            if "shortcut_always" in mut or mag1[best] < f32(0.875) * mag1[cand[1]]:
                return True, cand
        cand.append(best)
    return False, cand


def float_values(yr, yi):
    """stage 2 for all 320 lags: lag i = 8 a + b reads the 144 floats from sample 8 a on; float phi = 2 m + part meets tap
    k = m - b; ONE fma chain per sum from +0 in the order j, s', kk of phi = 16 j + 4 kk + s'"""
    lt = taps()[0]
    A = np.stack([yr, yi], axis=1).reshape(-1).astype(np.float32)
    i = np.arange(SYNC)
    a, b = i >> 3, i & 7
    ar, ai = np.zeros(SYNC, np.float32), np.zeros(SYNC, np.float32)
    zero = np.zeros(SYNC, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(9):
            for sp in range(4):
                for kk in range(4):
                    phi = 16 * j + 4 * kk + sp
                    m, part = phi >> 1, phi & 1
                    k = m - b
                    ok = (k >= 0) & (k < 64)
                    lr = np.where(ok, lt[np.clip(k, 0, 63), 0], zero)
                    li = np.where(ok, lt[np.clip(k, 0, 63), 1], zero)
                    cr = li if part else lr
                    ci = lr if part else np.where(ok, f32(0) - li, zero)
                    v = A[16 * a + phi]
                    ar = fma32(v, cr, ar)
                    ai = fma32(v, ci, ai)
        return ar, ai, fma32(ai, ai, ar * ar)


def top_four(cand, mag, mut=()):
    """the (up to) four largest candidates by float magnitude, ties -> lower lag, a NaN never a peak; -1: no such peak"""
    top = []
    key = {}
    for c in cand:
        v = mag[c]
        if np.isnan(v):
            if "nan_is_peak" not in mut:
                continue
            v = np.inf
        key[c] = float(v)
    for _ in range(4):
        left = [c for c in key if c not in top]
        if not left:
            top.append(-1)
            continue
        mx = max(key[c] for c in left)
        tied = sorted(c for c in left if key[c] == mx)
        top.append(tied[-1] if "top4_tie_high" in mut else tied[0])
    return top


def pair_search(top, mut=()):
    """App. A.3: pairs (i < k) of the top four in order; distance 64 ends the search, 63 / 65 are taken and the search
    goes on.  Returns (found distance or 0, frame start, lag of `first`, lag of `second`)"""
    found, fs, lo, hi = 0, SYNC, -1, -1
    for i in range(3):
        for k in range(i + 1, 4):
            if found == 64 and "last_pair_wins" not in mut:
                continue
            oi, ok = top[i], top[k]
            if oi < 0 or ok < 0:
                continue
            d = abs(oi - ok)
            if d == 64 or (d in (63, 65) and "no_63_65" not in mut):
                found, fs, lo, hi = d, min(oi, ok), min(oi, ok), max(oi, ok)
    return found, fs, lo, hi


def frame(slot, t, cfo_c, sincos, atan2, mut=(), L=None):
    """one trigger of a slot (or of a stream, with L = the samples up to the next trigger): everything between the trigger
    and the first FFT, as a dict"""
    slot = np.ascontiguousarray(slot, dtype=np.complex64).reshape(-1)
    L = min(slot.size - (t - 16), MAX_SAMPLES) if L is None else L
    out = dict(L=L, flags=F_DETECTED, frame_start=0, cfo_fine=f32(0), found=0)
    if L < SYNC + 63:
        out["flags"] |= F_TRUNCATED
        return out
    xr, xi = window(slot, t)
    yr, yi = derotate(xr, xi, cfo_c, sincos)
    E, scale, q, r = quantise(yr, yi, mut)
    mag1, cr, ci = int_magnitudes(q)
    short, cand = candidates(mag1, mut)
    ar, ai, mag = float_values(yr, yi)
    top = top_four(cand, mag, mut)
    found, fs, lo, hi = pair_search(top, mut)
    out.update(xr=xr, xi=xi, yr=yr, yi=yi, E=E, scale=scale, q=q, rint=r, mag1=mag1, shortcut=short, cand=cand,
               cand_re=ar[cand], cand_im=ai[cand], corr_re=ar, corr_im=ai, mag=mag, top=top,
               top_mag=np.array([mag[c] if c >= 0 else 0 for c in top], np.float32), found=found)
    if found:
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            a_re, a_im, b_re, b_im = ar[lo:lo + 1], ai[lo:lo + 1], ar[hi:hi + 1], ai[hi:hi + 1]
            pr = fma32(a_im, b_im, a_re * b_re)
            pi = fma32(a_im, b_re, -(a_re * b_im))
            ang = atan2(pi, pr)
            out.update(flags=F_DETECTED | F_SYNC, frame_start=fs, pr=pr[0], pi=pi[0],
                       cfo_fine=(ang / f32(64 if "divide_by_64" in mut else found)).astype(np.float32)[0])
    return out


def definition(slot, t, cfo_c):
    """the same search by its definition in float64: y = x exp(-j cfo_c m), corr[i] = sum conj(l[k]) y[i + k] over all 320
    lags, the four largest |corr| (lower lag first among equals), the pair search, arg(first conj(second)) / diff.
    Returns (found, frame_start, cfo_fine)."""
    xr, xi = window(slot, t)
    y = (xr.astype(np.float64) + 1j * xi.astype(np.float64)) * np.exp(-1j * float(cfo_c) * np.arange(WIN))
    l = lts64()
    corr = np.array([np.sum(np.conj(l) * y[i:i + 64]) for i in range(SYNC)])
    mag = np.abs(corr)
    order = sorted(range(SYNC), key=lambda i: (-mag[i], i))[:4]
    found, fs, lo, hi = pair_search(order)
    if not found:
        return 0, 0, 0.0
    return found, fs, float(np.angle(corr[lo] * np.conj(corr[hi]))) / found
