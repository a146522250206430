"""Joint detection over A sample-synchronous antennas restated: NUMERICS.md rule 24 in float32 NumPy.

Per antenna the summands are rule 3's -- a[n] = x[n] conj(x[n - 16]) by rule 2's first form, |x[n]|^2 = fma(im, im, re re) --;
they are added over the antenna index by a pairwise tree, per component, and the SUMS go through rule 3's blocked window
sums and its threshold comparison, unchanged.  Built from the pieces of tests/detect_ref.py (fma32, the scans, `above`,
sync_short); imports nothing of the product or the oracle.

`mutant` selects one of the three wrong readings of the rule that tests/test_detect_multi_ref.py pins:
"left-to-right sum" (((s0 + s1) + s2) + ... in place of the tree), "windows before the antenna sum" (every antenna's window
sums by rule 3, the tree over A[n] and P[n]) and "threshold per antenna OR-ed" (rule 3 per antenna, a sample is above when
it is above on any antenna)."""
import numpy as np

import detect_ref as dr
from detect_ref import _scan16, _shift_blocks, fma32

MUTANTS = ("left-to-right sum", "windows before the antenna sum", "threshold per antenna OR-ed")


def summands(x):
    """rule 3's summands of one antenna, padded to whole blocks of 16: (a_re, a_im, pw) float32 [16 nb]"""
    x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
    n = x.size
    nb = (n + 15) // 16
    xr = np.zeros(16 * nb, np.float32)
    xi = np.zeros(16 * nb, np.float32)
    xr[:n], xi[:n] = x.real, x.imag
    d_re = np.zeros_like(xr)
    d_im = np.zeros_like(xi)
    d_re[16:], d_im[16:] = xr[:-16], xi[:-16]
    c, s = d_re, -d_im
    return fma32(-xi, s, xr * c), fma32(xi, c, xr * s), fma32(xi, xi, xr * xr)


def tree_sum(parts, left_to_right=False):
    """the pairwise tree over the antenna index: neighbours are added level by level, an odd one out moves up as it is
    (3: (s0 + s1) + s2; 8: ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))).  float32 throughout."""
    v = [np.asarray(p, dtype=np.float32) for p in parts]
    if left_to_right:
        acc = v[0]
        for p in v[1:]:
            acc = acc + p
        return acc
    while len(v) > 1:
        nxt = [v[2 * i] + v[2 * i + 1] for i in range(len(v) // 2)]
        if len(v) & 1:
            nxt.append(v[-1])
        v = nxt
    return v[0]


def windows(v, back, n):
    """rule 3's blocked window sum of the summands v (float32 [16 nb]): the window reaches `back` blocks back (3: the 48
    samples of A, 4: the 64 of P)"""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 16)
    H = _scan16(v, False)
    S = _scan16(v, True)
    T = np.zeros_like(S)
    T[:, :15] = S[:, 1:]                                # T[r] = S[r + 1], T[15] = 0
    B = np.repeat(H[:, 15:16], 16, axis=1)              # block total
    acc = _shift_blocks(T, back)
    for d in range(back - 1, 0, -1):
        acc = acc + _shift_blocks(B, d)
    return (acc + H).reshape(-1)[:n]


def window_sums(xs, mutant=None):
    """rule 24: (Ar, Ai, P) float32 [n] of the antennas' complex64 streams xs (one length, from the stream origin)"""
    xs = [np.ascontiguousarray(x, dtype=np.complex64).reshape(-1) for x in xs]
    n = xs[0].size
    assert 1 <= len(xs) <= 8 and all(x.size == n for x in xs)
    if n == 0:
        z = np.zeros(0, np.float32)
        return z, z.copy(), z.copy()
    parts = [summands(x) for x in xs]
    if mutant == "windows before the antenna sum":
        return tuple(tree_sum([windows(p[c], back, n) for p in parts]) for c, back in ((0, 3), (1, 3), (2, 4)))
    ltr = mutant == "left-to-right sum"
    return tuple(windows(tree_sum([p[c] for p in parts], ltr), back, n) for c, back in ((0, 3), (1, 3), (2, 4)))


def bits(xs, thr, mutant=None):
    """the c > thr bits of rule 24: rule 3's comparison on the joint sums"""
    if mutant == "threshold per antenna OR-ed":
        out = None
        for x in xs:
            b = dr.above(*dr.window_sums(x), thr)[0]
            out = b if out is None else (out | b)
        return out
    return dr.above(*window_sums(xs, mutant), thr)[0]


def masks(b):
    """the bits as the device's 64-bit words: bit l of word t = sample 64 t + l"""
    b = np.asarray(b, dtype=bool)
    pad = np.zeros((b.size + 63) // 64 * 64, dtype=np.uint8)
    pad[:b.size] = b
    return np.packbits(pad.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1)


def detect(xs, thr, min_plateau, mutant=None):
    """the joint detect phase: (triggers int64 [k], Ar[triggers], Ai[triggers])"""
    Ar, Ai, _ = window_sums(xs, None if mutant == "threshold per antenna OR-ed" else mutant)
    t = np.asarray(dr.sync_short(bits(xs, thr, mutant), min_plateau), dtype=np.int64)
    return t, Ar[t], Ai[t]


def definition(xs):
    """the joint sums by their definition: the float64 sliding sums of every antenna (detect_ref.definition), added"""
    d = [dr.definition(x) for x in xs]
    return tuple(sum(c[k] for c in d) for k in range(3))


def abs_terms(xs):
    """per component the window's sum of absolute terms, float64: what a rounding of the float32 evaluation is relative
    to.  A summand's terms are its two products (|re re'| + |im im'| and so on)."""
    out = [0.0, 0.0, 0.0]
    for x in xs:
        x = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1).astype(np.complex128)
        xd = np.concatenate([np.zeros(16, np.complex128), x])[:x.size]
        t = (np.abs(x.real * xd.real) + np.abs(x.imag * xd.imag), np.abs(x.imag * xd.real) + np.abs(x.real * xd.imag),
             x.real * x.real + x.imag * x.imag)
        for k, w in enumerate((48, 48, 64)):
            pad = np.concatenate([np.zeros(w - 1), t[k]])
            out[k] = out[k] + np.lib.stride_tricks.sliding_window_view(pad, w).sum(axis=1)
    return tuple(out)
