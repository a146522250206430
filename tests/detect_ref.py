"""The detect phase restated: NUMERICS.md rule 3 (window sums, threshold comparison) in float32 NumPy, the same sums by
their float64 definition, and sync_short's SEARCH / COPY state machine as the scalar loop of SURVEY.md App. A.2.

Written from those two texts.  Imports nothing of the product or the oracle (tests/test_detect_rows.py checks that).
Python 3.10 has no math.fma: `fma32` is an exact float32 fused multiply-add built from float64 operations."""
import numpy as np

MIN_GAP = 480               # WIFIRX_MIN_GAP
MAX_SAMPLES = 540 * 80      # WIFIRX_MAX_SAMPLES

f32 = np.float32


def fma32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, for float32 operands (arrays or scalars).
    The product of two float32 values is exact in float64 (48 significant bits, exponent in range).  The sum p + c is
    rounded to float64 and TwoSum gives its error exactly; where there is one, the float64 value is moved to the
    neighbour with an odd last bit (round to odd), after which the rounding to float32 (29 bits fewer) cannot be a
    double rounding."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        even = (np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, other, s)
        return s.astype(np.float32)


def _scan16(v, suffix):
    """inclusive Kogge-Stone scan over the last axis (16): steps 1, 2, 4, 8, v[i] = v[i -+ k] + v[i] (float32)"""
    v = v.copy()
    for k in (1, 2, 4, 8):
        w = v.copy()
        if suffix:
            w[..., :16 - k] = v[..., k:] + v[..., :16 - k]
        else:
            w[..., k:] = v[..., :16 - k] + v[..., k:]
        v = w
    return v


def _shift_blocks(v, d):
    """v[m - d] along axis 0, +0 where there is no such block"""
    out = np.zeros_like(v)
    if d < v.shape[0]:
        out[d:] = v[:v.shape[0] - d]
    return out


def window_sums(x, tail=1):
    """rule 3: (Ar, Ai, P) float32 [n] of the complex64 stream x, which starts at the stream origin (x[n < 0] = 0).
    a[n] = x[n] * conj(x[n - 16]) by rule 2's first form with (c, s) = (Re, -Im) of x[n - 16]; |x|^2 = fma(im, im, re re).
    tail: T[r] = S[r + tail]; 1 is the rule, 0 (`T[r] = S[r]`, windows of 49 / 65) and 2 (windows of 47 / 63) are the
    mutants of tests/test_detect_rows.py."""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n = x.size
    nb = (n + 15) // 16
    if nb == 0:
        z = np.zeros(0, np.float32)
        return z, z.copy(), z.copy()
    xr = np.zeros(16 * nb, np.float32)
    xi = np.zeros(16 * nb, np.float32)
    xr[:n], xi[:n] = x.real, x.imag
    dr = np.zeros_like(xr)
    di = np.zeros_like(xi)
    dr[16:], di[16:] = xr[:-16], xi[:-16]
    c, s = dr, -di
    a_re = fma32(-xi, s, xr * c)
    a_im = fma32(xi, c, xr * s)
    pw = fma32(xi, xi, xr * xr)
    out = []
    for v, back in ((a_re, 3), (a_im, 3), (pw, 4)):
        v = v.reshape(nb, 16)
        H = _scan16(v, False)
        S = _scan16(v, True)
        T = np.zeros_like(S)
        T[:, :16 - tail] = S[:, tail:]                      # T[r] = S[r + 1], T[15] = 0
        B = np.repeat(H[:, 15:16], 16, axis=1)              # block total
        acc = _shift_blocks(T, back)
        for d in range(back - 1, 0, -1):
            acc = acc + _shift_blocks(B, d)
        out.append((acc + H).reshape(-1)[:n])
    return out[0], out[1], out[2]


def above(Ar, Ai, P, thr, ge=False):
    """the c > thr bits as rule 3 compares them: fma(Ai, Ai, Ar Ar) > (thr P) (thr P), all float32.  thr: a scalar or one
    value per sample.  Returns (bits, m2, tp2).  ge: the mutant `>=` (tests/test_detect_rows.py)."""
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float32), np.shape(P))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m2 = fma32(Ai, Ai, Ar * Ar)
        tp = thr * P
        tp2 = tp * tp
        return (m2 >= tp2) if ge else (m2 > tp2), m2, tp2


def definition(x, win_a=48, win_p=64):
    """A and P as their definition: plain float64 sliding sums of x[n] conj(x[n - 16]) over 48 and of |x|^2 over 64 samples"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1).astype(np.complex128)
    xd = np.concatenate([np.zeros(16, np.complex128), x])[:x.size]
    a = x * np.conj(xd)
    p = x.real * x.real + x.imag * x.imag

    def slide(v, w):            # every window summed on its own: no running sum whose earlier terms could linger
        pad = np.concatenate([np.zeros(w - 1), v])
        return np.lib.stride_tricks.sliding_window_view(pad, w).sum(axis=1) if v.size else v
    return slide(a.real, win_a), slide(a.imag, win_a), slide(p, win_p)


def sync_short(bits, min_plateau, first_only=False, plateau_le=False, gap_ge=False):
    """SURVEY.md App. A.2 as a scalar loop over the c > thr bits.  Returns the list of trigger indices.
    plateau_le / gap_ge: the mutants `plateau <= min_plateau` and `copied >= MIN_GAP`."""
    bits = np.asarray(bits, dtype=bool).tolist()
    trig = []
    search, plateau, copied = True, 0, 0
    i, n = 0, len(bits)
    while i < n:
        if search:
            if bits[i]:
                if (plateau <= min_plateau) if plateau_le else (plateau < min_plateau):
                    plateau += 1
                else:                       # the trigger sample is not consumed: COPY sees it again
                    trig.append(i)
                    if first_only:
                        break
                    search, copied, plateau = False, 0, 0
                    continue
            else:
                plateau = 0
            i += 1
        else:
            if bits[i]:
                if (plateau <= min_plateau) if plateau_le else (plateau < min_plateau):
                    plateau += 1
                elif (copied >= MIN_GAP) if gap_ge else (copied > MIN_GAP):
                    trig.append(i)          # returns before copying the item: it is seen again with the new counters
                    copied, plateau = 0, 0
                    continue
            else:
                plateau = 0
            copied += 1
            i += 1
            if copied == MAX_SAMPLES:
                search = True
    return trig


def detect(x, thr, min_plateau, first_only=False):
    """the whole restated detect phase: (triggers int32 [k], Ar[triggers], Ai[triggers]) of stream x"""
    Ar, Ai, P = window_sums(x)
    bits = above(Ar, Ai, P, thr)[0]
    t = np.asarray(sync_short(bits, min_plateau, first_only), dtype=np.int64)
    return t.astype(np.int32), Ar[t], Ai[t]
