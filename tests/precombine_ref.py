"""NUMERICS.md rule 33 restated in NumPy float32, value for value: pre-detection combining of A antennas' sample rows into one
row set (wifirx_precombine, wr_precombine.hip).  Fused steps go through detect_ref.fma32; everything else is float32 NumPy with
one rounding per written operation.  direct() is the float64 definition the rule is held against.

    combine(xs, slot_len, iters=2) -> (y [n_slots, slot_len] complex64, weights [n_slots, A] complex64, stats [n_slots] STATS_DTYPE)

`mutant` runs a deliberately wrong variant of one clause (tests/test_precombine_ref.py: each must fail the test named for it):
    lane_sum   the 64 lanes of a wave added left to right instead of by the xor butterfly
    ref0       the reference antenna fixed to 0
    noconj     the stream formed with v instead of conj(v)
    nonorm     the weights left at their covariance scale (no division by the norm)
    norot      no rotation of the reference antenna's weight onto the real axis"""
import numpy as np

from detect_ref import fma32

f32 = np.float32
MAX_ANT, MAX_ITERS, WAVES = 8, 4, 4
DEGENERATE = 1
STATS_DTYPE = np.dtype([("lambda", "<f4"), ("trace", "<f4"), ("ref", "<u4"), ("flags", "<u4")])
assert STATS_DTYPE.itemsize == 16
MUTANTS = ("lane_sum", "ref0", "noconj", "nonorm", "norot")


def _parts(x):
    x = np.asarray(x, dtype=np.complex64)
    return np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)


def _butterfly(v):
    """the fold of the last axis (64 lanes): lane xor 32, 16, 8, 4, 2, 1, float32; every lane ends with the sum"""
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in (32, 16, 8, 4, 2, 1):
            v = (v + v[..., lanes ^ m]).astype(f32)
    return v[..., 0]


def _left_to_right(v):
    acc = v[..., 0]
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(1, 64):
            acc = (acc + v[..., l]).astype(f32)
    return acc


def covariance(xs, slot_len, mutant=None):
    """item 1: R [n_slots, A, A] as (re, im) float32 arrays.  Sample n = 64 t + l belongs to chain (t mod 4, l); a chain starts
    at +0 and takes its terms ascending in t, each term continuing rule 2's product form into the accumulator:
        diagonal       acc = fma(im, im, fma(re, re, acc))
        a < b, re      acc = fma(a.im, b.im, fma(a.re, b.re, acc))
        a < b, im      acc = fma(a.im, b.re, fma(a.re, -b.im, acc))
    Then the 64 lanes of a chain set (one wave) fold by the xor butterfly, and the four folded sums add as (w0 + w1) + (w2 + w3)."""
    A = len(xs)
    parts = [_parts(np.asarray(x).reshape(-1, slot_len)) for x in xs]
    n = parts[0][0].shape[0]
    tiles = slot_len // 64
    steps = (tiles + WAVES - 1) // WAVES
    pad = steps * WAVES - tiles
    tiled = []
    for re, im in parts:                # [n, steps, 4, 64]; the tiles behind the slot are never added (masked below)
        re = np.concatenate([re.reshape(n, tiles, 64), np.zeros((n, pad, 64), f32)], axis=1).reshape(n, steps, WAVES, 64)
        im = np.concatenate([im.reshape(n, tiles, 64), np.zeros((n, pad, 64), f32)], axis=1).reshape(n, steps, WAVES, 64)
        tiled.append((re, im))
    fold = _left_to_right if mutant == "lane_sum" else _butterfly
    Rre = np.zeros((n, A, A), f32)
    Rim = np.zeros((n, A, A), f32)
    for a in range(A):
        for b in range(a, A):
            cr = np.zeros((n, WAVES, 64), f32)
            ci = np.zeros((n, WAVES, 64), f32)
            for k in range(steps):
                valid = (np.arange(WAVES) + WAVES * k < tiles)[None, :, None]
                are, aim = tiled[a][0][:, k], tiled[a][1][:, k]
                bre, bim = tiled[b][0][:, k], tiled[b][1][:, k]
                if a == b:
                    cr = np.where(valid, fma32(aim, aim, fma32(are, are, cr)), cr)
                else:
                    cr = np.where(valid, fma32(aim, bim, fma32(are, bre, cr)), cr)
                    ci = np.where(valid, fma32(aim, bre, fma32(are, -bim, ci)), ci)
            with np.errstate(invalid="ignore", over="ignore"):
                w = fold(cr)
                Rre[:, a, b] = ((w[:, 0] + w[:, 1]).astype(f32) + (w[:, 2] + w[:, 3]).astype(f32)).astype(f32)
                if a != b:
                    w = fold(ci)
                    im = ((w[:, 0] + w[:, 1]).astype(f32) + (w[:, 2] + w[:, 3]).astype(f32)).astype(f32)
                    Rim[:, a, b] = im
                    Rre[:, b, a] = Rre[:, a, b]
                    Rim[:, b, a] = -im
    return Rre, Rim


def _matvec(Rre, Rim, vre, vim):
    """u_a = sum_b R_ab v_b per slot (R [n, A, A], v [n, A]): per row a chain from +0, ascending in b:
    re = fma(-x.im, s, fma(x.re, c, re)), im = fma(x.im, c, fma(x.re, s, im)) with x = R_ab and (c, s) = v_b"""
    n, A = vre.shape
    ure, uim = np.zeros((n, A), f32), np.zeros((n, A), f32)
    for a in range(A):
        re, im = np.zeros(n, f32), np.zeros(n, f32)
        for b in range(A):
            re = fma32(-Rim[:, a, b], vim[:, b], fma32(Rre[:, a, b], vre[:, b], re))
            im = fma32(Rim[:, a, b], vre[:, b], fma32(Rre[:, a, b], vim[:, b], im))
        ure[:, a], uim[:, a] = re, im
    return ure, uim


def _normalise(ure, uim):
    """v = u / sqrt(sum |u_a|^2) per slot: the sum an fma chain from +0 (re then im, ascending a), the root and the divisions
    correctly rounded; also whether the norm is finite and > 0 (where it is not, v is not to be used)"""
    s = np.zeros(ure.shape[0], f32)
    for a in range(ure.shape[1]):
        s = fma32(ure[:, a], ure[:, a], s)
        s = fma32(uim[:, a], uim[:, a], s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nrm = np.sqrt(s.astype(f32))
        return (ure / nrm[:, None]).astype(f32), (uim / nrm[:, None]).astype(f32), np.isfinite(nrm) & (nrm > 0)


def slot_weights(Rre, Rim, iters, mutant=None):
    """items 2, 3 and 5 on R [n, A, A]: (vre, vim [n, A], stats [n]).  Every slot is worked on alone; the slots that turn out
    degenerate on the way are overwritten at the end."""
    n, A = Rre.shape[:2]
    rows = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        trace, top, r = Rre[:, 0, 0].copy(), Rre[:, 0, 0].copy(), np.zeros(n, np.int64)
        for a in range(1, A):
            d = Rre[:, a, a]
            trace = (trace + d).astype(f32)
            rep = d > top                       # ties keep the lower index; a NaN neither replaces nor is replaced
            top, r = np.where(rep, d, top), np.where(rep, a, r)
        if mutant == "ref0":
            r[:] = 0
        ok = np.isfinite(trace) & (trace > 0)
        ure, uim = Rre[rows, :, r], Rim[rows, :, r]
        if mutant == "nonorm":
            vre, vim = ure, uim
            for _ in range(iters):
                vre, vim = _matvec(Rre, Rim, vre, vim)
        else:
            vre, vim, good = _normalise(ure, uim)
            ok &= good
            for _ in range(iters):
                vre, vim, good = _normalise(*_matvec(Rre, Rim, vre, vim))
                ok &= good
        if mutant != "norot":
            p, q = vre[rows, r], vim[rows, r]
            m = np.sqrt(fma32(q, q, (p * p).astype(f32)))
            ok &= np.isfinite(m) & (m > 0)
            c, s = (p / m).astype(f32)[:, None], (-q / m).astype(f32)[:, None]
            # v_a (c + js) by rule 2's first form; the reference antenna's weight is (m, +0) exactly
            vre, vim = fma32(-vim, s, (vre * c).astype(f32)), fma32(vim, c, (vre * s).astype(f32))
            vre[rows, r], vim[rows, r] = m, 0
        wre, wim = _matvec(Rre, Rim, vre, vim)
        lam = np.zeros(n, f32)
        for a in range(A):
            lam = fma32(vre[:, a], wre[:, a], lam)
            lam = fma32(vim[:, a], wim[:, a], lam)
    vre, vim = vre.copy(), vim.copy()
    vre[~ok], vim[~ok] = 0, 0
    vre[~ok, 0] = 1
    stats = np.zeros(n, STATS_DTYPE)
    stats["lambda"], stats["trace"] = np.where(ok, lam, f32(0)), trace
    stats["ref"], stats["flags"] = np.where(ok, r, 0), np.where(ok, 0, DEGENERATE)
    return vre, vim, stats


def combine(xs, slot_len, iters=2, mutant=None):
    """rule 33 on A arrays of n_slots * slot_len complex64 samples"""
    A = len(xs)
    assert 1 <= A <= MAX_ANT and 0 <= iters <= MAX_ITERS and slot_len % 64 == 0 and 64 <= slot_len <= 65536
    xs = [np.asarray(x, dtype=np.complex64).reshape(-1, slot_len) for x in xs]
    n = xs[0].shape[0]
    weights = np.zeros((n, A), np.complex64)
    stats = np.zeros(n, STATS_DTYPE)
    if A == 1:                                  # item 5: no sums are formed
        weights[:, 0] = 1
        return xs[0].copy(), weights, stats
    Rre, Rim = covariance(xs, slot_len, mutant)
    vre, vim, stats = slot_weights(Rre, Rim, iters, mutant)
    weights.real, weights.imag = vre, vim
    sign = f32(-1) if mutant == "noconj" else f32(1)
    # item 4: conj(v_0) x_0 by rule 2's second form, then one fma pair per further antenna, ascending
    x0re, x0im = _parts(xs[0])
    c, s = vre[:, :1], vim[:, :1] * sign
    with np.errstate(invalid="ignore", over="ignore"):
        re = fma32(s, x0im, (c * x0re).astype(f32))
        im = fma32(-s, x0re, (c * x0im).astype(f32))
    for a in range(1, A):
        xre, xim = _parts(xs[a])
        c, s = vre[:, a:a + 1], vim[:, a:a + 1] * sign
        re = fma32(s, xim, fma32(c, xre, re))
        im = fma32(-s, xre, fma32(c, xim, im))
    y = np.empty((n, slot_len), np.complex64)
    y.real, y.imag = re, im
    deg = (stats["flags"] & DEGENERATE) != 0
    y[deg] = xs[0][deg]                         # item 5: bit for bit (a view copy: NaN payloads and signed zeros survive)
    return y, weights, stats


def direct(xs, slot_len, iters=None):
    """the float64 definition: R = sum_n x x^H per slot; iters None: the principal eigenvector (iters -> infinity), otherwise the
    same finite iteration from the column of the strongest antenna; unit norm, the reference antenna's weight real and >= 0.
    Returns (y, v, lambda, trace, ref) in complex128 / float64."""
    X = np.stack([np.asarray(x, dtype=np.complex128).reshape(-1, slot_len) for x in xs], axis=1)       # [n, A, S]
    R = np.einsum("nas,nbs->nab", X, X.conj())
    diag = np.real(np.einsum("naa->na", R))
    ref = np.argmax(diag, axis=1)
    n, A = diag.shape
    v = np.zeros((n, A), np.complex128)
    for i in range(n):
        if iters is None:
            _, vec = np.linalg.eigh(R[i])
            u = vec[:, -1]
        else:
            u = R[i][:, ref[i]]
            u = u / np.linalg.norm(u)
            for _ in range(iters):
                u = R[i] @ u
                u = u / np.linalg.norm(u)
        u = u * np.exp(-1j * np.angle(u[ref[i]]))
        v[i] = u / np.linalg.norm(u)
    y = np.einsum("na,nas->ns", v.conj(), X)
    lam = np.real(np.einsum("na,nab,nb->n", v.conj(), R, v))
    return y, v, lam, diag.sum(axis=1), ref
