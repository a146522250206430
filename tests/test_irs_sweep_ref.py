"""NUMERICS.md rule 26 on the host (tests/irs_sweep_ref.py) and the codebooks of wifirx.irs, without a device:
  * the chain against the same sum in float64 within (2 N + 1) 2^-24 sum |e_n| per part; the zero-fill terms; the tie rule;
  * the winner's taps against rule 25 with psi = codebook[best] within the rule's bound (largest ratio printed);
  * dft_codebook: unit modulus, orthogonal rows at over = 1, the scalloping bound at over = 2; quantize; traverse_codebook at
    entries worked out by hand."""
import math

import numpy as np
import pytest

import irs_ref
import irs_sweep_ref as sr
from wifirx import irs

F32 = np.float32


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def unit(rng, *shape):
    return np.exp(1j * rng.uniform(-np.pi, np.pi, shape)).astype(np.complex64)


@pytest.mark.parametrize("N", [1, 3, 64, 257])
def test_chain_against_float64(N):
    rng = np.random.default_rng(N)
    e, cb = crandn(rng, 6, N), unit(rng, 9, N)
    c_re, c_im = sr.coefficients(cb)
    A = sr.interleave(*irs_ref.parts(e))
    assert A.shape[-1] == c_re.shape[-1] == -(-2 * N // 4) * 4 and A.dtype == c_re.dtype == F32
    y = sr.chain(A, c_re).astype(np.float64) + 1j * sr.chain(A, c_im).astype(np.float64)
    exact = e.astype(np.complex128) @ cb.astype(np.complex128).T
    # 2 N roundings of a chain whose terms sum to at most sum |e_n| |psi_n| = sum |e_n| in magnitude (Cauchy-Schwarz per
    # element), and one more unit for the codebook's modulus, which is 1 only to 2^-24
    lim = (2 * N + 1) * 2.0 ** -24 * np.abs(e.astype(np.complex128)).sum(axis=1)[:, None]
    ratio = max(float((np.abs(y.real - exact.real) / lim).max()), float((np.abs(y.imag - exact.imag) / lim).max()))
    print("N = %d: chain against float64, largest error / bound = %.4f" % (N, ratio))
    assert ratio <= 1.0


def test_zero_fill_terms():
    """the fill terms are part of the chain: fma(+0, +0, sum) turns a -0 sum into +0 and does nothing else"""
    for N in (1, 2, 3, 4):
        cb = unit(np.random.default_rng(0), 2, N)
        c_re, c_im = sr.coefficients(cb)
        P = -(-2 * N // 4) * 4
        assert c_re.shape == (2, P) and not np.signbit(c_re[:, 2 * N:]).any() and (c_im[:, 2 * N:] == 0).all()
        assert np.array_equal(c_re[:, 1:2 * N:2], -cb.imag) and np.array_equal(c_im[:, 0:2 * N:2], cb.imag)
    tiny = F32(1e-30)
    # a product that underflows to -0, then terms that keep the sign: -0 after 2 N = 4 terms, and no fill follows
    e = (np.array([[-tiny, F32(-0.0)]], F32), np.array([[F32(0.0), F32(-0.0)]], F32))
    cb = np.array([[tiny + 0j, 1 - 1j]], np.complex64)
    c_re, _ = sr.coefficients(cb)
    assert np.signbit(sr.chain(sr.interleave(*e), c_re)).all()
    # the same first element alone (N = 1) and with two more (N = 3): 2 N is no multiple of 4, the fill makes it +0
    for n in (1, 3):
        en = (np.concatenate([e[0], np.full((1, n - 1), F32(-0.0))], axis=1)[:, :n], np.concatenate([e[1], np.full((1, n - 1), F32(-0.0))], axis=1)[:, :n])
        en[1][0, 0] = F32(0.0)
        cbn = np.concatenate([cb, np.full((1, n - 1), 1 - 1j, np.complex64)], axis=1)[:, :n]
        y = sr.chain(sr.interleave(*en), sr.coefficients(cbn)[0])
        assert (y == 0).all() and not np.signbit(y).any(), n


def test_tie_rule():
    nan = F32(np.nan)
    p = np.array([[1, 3, 3, 2], [nan, 0, nan, 0], [nan, nan, nan, nan], [0, 0, 0, 0], [2, nan, 5, 5], [np.inf, np.inf, 1, nan]], F32)
    assert sr.winner(p).tolist() == [1, 1, 0, 0, 2, 0] and sr.winner(p).dtype == np.uint16
    # through the whole rule: two identical entries, an entry holding a NaN, all entries NaN
    rng = np.random.default_rng(3)
    N, L, n_sets = 5, 2, 6
    e, hd = irs_ref.parts(crandn(rng, n_sets, L, N)), irs_ref.parts(crandn(rng, n_sets, L))
    scale = np.array([1.0, 0.5], F32)
    two = unit(rng, 2, N)
    r = sr.from_parts(e, hd, scale, np.stack([two[0], two[1], two[1], two[0]]))
    assert (r["best"] < 2).all() and np.array_equal(r["power"][:, 0], r["power"][:, 3]) and set(r["best"].tolist()) == {0, 1}
    for at in (0, 2):
        cb = np.stack([two[0], two[1], two[0]])
        cb[at, 2] = np.nan
        r = sr.from_parts(e, hd, scale, cb)
        assert np.isnan(r["power"][:, at]).all() and (r["best"] != at).all() and np.isfinite(r["taps"]).all()
    cb = np.stack([two[0], two[1]])
    cb[:, 0] = np.nan
    r = sr.from_parts(e, hd, scale, cb)
    assert np.isnan(r["power"]).all() and (r["best"] == 0).all()


@pytest.mark.parametrize("N", [3, 65, 257])
def test_winner_against_rule_25(N):
    rng = np.random.default_rng(700 + N)
    L, n_sets, K = 3, 5, 17
    a, b, d = crandn(rng, N), crandn(rng, N), crandn(rng, 1)[0]
    pdp = np.exp(-np.arange(L) / 3.0).astype(F32)
    sc = crandn(rng, n_sets * L, 2 * N + 1)
    cb = unit(rng, K, N)
    worst = 0.0
    for k_factor, dg in [(0.0, 1.0), (10.0, 1.0), (3.0, 0.0)]:
        kw = dict(gain=1.3, k_factor=k_factor, direct_gain=dg, scatter=sc)
        s = sr.irs_sweep(n_sets, pdp, a, b, d, codebook=cb, **kw)
        assert np.array_equal(s["taps"], np.take_along_axis(s["all_taps"], s["best"].astype(np.intp)[:, None, None], 2)[..., 0])
        assert np.array_equal(s["best"], np.argmax(s["power"], axis=1))
        t = irs_ref.irs_taps(n_sets, pdp, a, b, d, psi=cb[s["best"]], **kw)
        assert np.array_equal(t["elems"], s["elems"])           # one scene, the same element bits
        scale = np.array([F32(math.sqrt(float(p)) * float(F32(1.3))) for p in pdp], F32)
        lim = sr.bound(s["direct"], s["elems"][:, :, 0, :], s["elems"][:, :, 1, :], scale)
        err = np.abs(s["taps"].astype(np.complex128) - t["taps"].astype(np.complex128))
        worst = max(worst, float((err / lim).max()))
        assert (err <= lim).all(), (k_factor, dg)
    print("N = %d: winner's taps against rule 25, largest error / bound = %.4f" % (N, worst))


# ---- the codebooks ----

def test_dft_codebook_unit_modulus_and_orthogonal():
    for S in (1, 2, 4, 8):
        N = S * S
        b2r, _, _ = irs.los(S, [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5], [S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0])
        for los_a in (None, b2r):
            cb = irs.dft_codebook(S, los_a)
            assert cb.dtype == np.complex64 and cb.shape == (N, N)
            assert np.abs(np.abs(cb.astype(np.complex128)) - 1).max() <= 2.0 ** -23
            gram = cb.astype(np.complex128) @ np.conj(cb.astype(np.complex128)).T
            assert np.abs(gram - N * np.eye(N)).max() <= N * 2.0 ** -20        # N terms, each rounded to complex64
        over = irs.dft_codebook(S, b2r, over=2)
        assert over.shape == (4 * N, N) and np.abs(np.abs(over) - 1).max() <= 2.0 ** -22
        # entry k = i M + j: the even-indexed beams of the 2x grid are the 1x grid
        M = 2 * S
        k1 = (2 * np.arange(S)[:, None] * M + 2 * np.arange(S)[None, :]).reshape(-1)
        assert np.abs(over[k1] - irs.dft_codebook(S, b2r)).max() <= 2.0 ** -20
    with pytest.raises(ValueError):
        irs.dft_codebook(0)
    with pytest.raises(ValueError):
        irs.dft_codebook(4, np.ones(15))


def test_dft_codebook_scalloping_bound():
    """over = 2, pure line of sight: the cascade gain of entry (i, j) is |D(pi (dx - u_i))| |D(pi (dy - u_j))| with the Dirichlet
    kernel D(x) = sin(S x / 2) / sin(x / 2) and (dx, dy) the user's direction cosines.  The grid's step in u is 2 / M = 1 / S, so
    some u_i lies within 1 / (2 S) of dx (the grid is periodic in u with period 2): |x| <= pi / (2 S), where
    D(x) >= sin(pi / 4) / sin(pi / (4 S)) >= sin(pi / 4) 4 S / pi = (2 sqrt(2) / pi) S.  Both axes: the best entry reaches at
    least (8 / pi^2) N = 0.81 N of the aligned sum N, a scalloping loss of at most 1.8 dB (over = 1: (2 / pi)^2 N, 3.9 dB)."""
    S = 8
    N = S * S
    irs_pos, ap_pos = [0.015, 0.015, 0], [S * 0.015, S * 0.015, 4.5]
    for user in ([S * 0.015 + 0.3, S * 0.015 - 0.2, 1.0], [-1.0, 2.0, 0.7], [0.5, 0.05, 3.0]):
        b2r, r2u, _ = irs.los(S, irs_pos, ap_pos, user)
        for over, floor in ((2, 8 / math.pi ** 2), (1, 4 / math.pi ** 2)):
            cb = irs.dft_codebook(S, b2r, over=over).astype(np.complex128)
            gain = np.abs((b2r[None, :] * cb * r2u[None, :]).sum(axis=1))
            print("user %r, over = %d: best entry reaches %.4f N (floor %.4f N)" % (user, over, gain.max() / N, floor))
            assert gain.max() >= floor * N - N * 2.0 ** -22         # the entries are rounded to complex64
            assert gain.max() <= N * (1 + 2.0 ** -22)


def test_quantize():
    rng = np.random.default_rng(5)
    ang = rng.uniform(-np.pi, np.pi, (7, 33))
    psi = (rng.uniform(0.2, 2.0, ang.shape) * np.exp(1j * ang)).astype(np.complex64)
    for bits in (1, 2, 3):
        q = irs.quantize(psi, bits)
        codes = irs.align_codes(psi.real, -psi.imag, 0, 0, bits)
        assert q.dtype == np.complex64 and q.shape == psi.shape
        assert np.array_equal(q, irs.PHASES[codes.astype(np.intp) << (3 - bits)])
        assert np.array_equal(irs.quantize(q, bits), q)           # idempotent
        off = np.angle(q.astype(np.complex128) * np.conj(psi.astype(np.complex128)))
        assert np.abs(off).max() <= np.pi / (1 << bits) + 1e-6    # the nearest table phase
    # the codebooks use it
    cb = irs.dft_codebook(4, over=2, bits=2)
    assert np.array_equal(cb, irs.quantize(irs.dft_codebook(4, over=2), 2)) and set(np.unique(cb).tolist()) <= {1, 1j, -1, -1j}
    with pytest.raises(ValueError):
        irs.quantize(psi, 4)


def test_traverse_codebook_at_hand_computed_entries():
    """scale 2, interval 0.03, surface corner (0.015, 0.015, 0), AP (0.24, 0.24, 0.5), accuracy 3: theta, phi in {-pi/2, 0, pi/2}.
    Element n = ix 2 + iy sits at x = 0.015 + 0.03 ix, y = 0.015 + 0.03 iy; wave number 2 pi 5e9 / 3e8."""
    cb = irs.traverse_codebook(2, 0.03, [0.015, 0.015, 0], [0.24, 0.24, 0.5], accuracy=3)
    assert cb.dtype == np.complex64 and cb.shape == (9, 4)
    w = 2 * math.pi * 5e9 / 3e8
    xy = {0: (0.015, 0.015), 1: (0.015, 0.045), 2: (0.045, 0.015), 3: (0.045, 0.045)}
    dist = {n: math.sqrt((x - 0.24) ** 2 + (y - 0.24) ** 2 + 0.25) for n, (x, y) in xy.items()}
    assert abs(dist[0] - 0.5926634795564849) < 1e-12 and abs(dist[3] - 0.5710078808562975) < 1e-12
    hand = {
        (4, 0): w * dist[0],                                  # theta = 0, phi = 0: the distance alone
        (5, 2): w * (dist[2] - xy[2][0]),                     # theta = 0, phi = pi/2: the other branch, D - sin(phi) x
        (3, 3): w * (dist[3] + xy[3][0]),                     # theta = 0, phi = -pi/2
        (1, 1): w * (dist[1] + xy[1][1]),                     # theta = -pi/2, phi = 0: sin(theta) cos(phi) = -1 goes with y
        (7, 2): w * (dist[2] - xy[2][1]),                     # theta = pi/2, phi = 0
        (8, 1): w * (dist[1] - xy[1][0]),                     # theta = pi/2, phi = pi/2: sin sin = 1 goes with x (cos = 6e-17)
        (6, 3): w * (dist[3] + xy[3][0]),                     # theta = pi/2, phi = -pi/2
    }
    for (k, n), pha in hand.items():
        assert abs(complex(cb[k, n]) - complex(math.cos(pha), math.sin(pha))) <= 1e-6, (k, n)
    assert abs(cb[5, 1] - cb[5, 0] * np.exp(1j * w * (dist[1] - dist[0]))) <= 1e-6       # theta = 0: y enters through D alone
    q = irs.traverse_codebook(2, 0.03, [0.015, 0.015, 0], [0.24, 0.24, 0.5], accuracy=3, bits=3)
    assert np.array_equal(q, irs.quantize(cb, 3))
    assert irs.traverse_codebook(16, 0.03, [0.015, 0.015, 0], [0.24, 0.24, 0.5]).shape == (100, 256)
