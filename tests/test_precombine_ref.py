"""tests/precombine_ref.py (NUMERICS.md rule 33 in NumPy float32) against its float64 definition within item 6's bound, every
clause of the rule on the rows of tests/precombine_rows.py, the array gain on a frame through known flat gains, and five mutants
of the reference, each of which a named test here must catch.

`python tests/test_precombine_ref.py` writes the mutants' record, profiles/precombine_mutations.txt."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                  # run as a script: what tests/conftest.py does for pytest
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

import precombine_ref as pr
import precombine_rows as rows
from detect_ref import fma32

F32 = np.float32
EPS = 2.0 ** -24


def sum_roundings(slot_len):
    """roundings on the way of a term to a component of R: two fused steps per term of its chain (ceil(tiles / 4) terms), six
    butterfly levels, two additions over the waves"""
    tiles = slot_len // 64
    return 2 * ((tiles + 3) // 4) + 8


def weight_bound(X, iters, slot_len):
    """Item 6's bound on || v32 - v64 ||_2 for one slot, from float64 quantities of the INPUT alone (X [A, S] complex128).
    With u = 2^-24, c = sum_roundings and tr = trace R: every entry of R is off by at most c u sum_n |x_a||x_b| <= c u
    sqrt(R_aa R_bb), so || dR ||_F <= c u tr; a matrix-vector product adds 2 A fused roundings per row on terms |R_ab||v_b|,
    at most 2 A u || R ||_F <= 2 A u tr in norm; a normalisation adds 2 A fused steps, a root and a division: (2 A + 2) u
    relative.  The map v -> R v / || R v || has the derivative (I - f f^H) R / || R v ||, of norm <= lambda_1 / || R v ||, so
        e_0     = (c + 2 A + 2) u tr / || R e_r ||
        e_(k+1) = (lambda_1 / || R v_k ||) e_k + (c + 2 A) u tr / || R v_k || + (2 A + 2) u
    and the rotation adds 4 u."""
    A = X.shape[0]
    R = X @ X.conj().T
    tr = float(np.real(np.trace(R)))
    lam1 = float(np.linalg.eigvalsh(R)[-1])
    r = int(np.argmax(np.real(np.diag(R))))
    c = sum_roundings(slot_len)
    col = R[:, r]
    e = (c + 2 * A + 2) * EPS * tr / np.linalg.norm(col)
    v = col / np.linalg.norm(col)
    for _ in range(iters):
        w = R @ v
        nw = np.linalg.norm(w)
        e = (lam1 / nw) * e + (c + 2 * A) * EPS * tr / nw + (2 * A + 2) * EPS
        v = w / nw
    return e + 4 * EPS


# ---- the checks: each takes the mutant it runs the reference with (None: the rule) -------------------------------------------

def check_against_float64(mutant=None, report=None):
    """R, the weights and the stream against direct(): every component of R within sum_roundings 2^-24 sum |terms|; the weights
    within weight_bound of the same finite iteration in float64; every component of y within 2 A 2^-24 sum |terms| of
    sum_a conj(v_a) x_a formed in float64 from the float32 weights (2 A terms per component, at most 2 A fused steps each)."""
    for A, S, iters in ((2, 64, 0), (2, 1472, 2), (3, 320, 1), (4, 4608, 2), (8, 1472, 4), (8, 128, 0)):
        n = 3
        xs = rows.build("scene", A, S, n, seed=7)
        y, v, st = pr.combine(xs, S, iters, mutant=mutant)
        Rre, Rim = pr.covariance(xs, S, mutant)
        X = np.stack([x.astype(np.complex128) for x in xs], axis=1)                 # [n, A, S]
        R64 = np.einsum("nas,nbs->nab", X, X.conj())
        absum = np.einsum("nas,nbs->nab", np.abs(X.real) + np.abs(X.imag), np.abs(X.real) + np.abs(X.imag))
        errR = np.maximum(np.abs(Rre - R64.real), np.abs(Rim - R64.imag)) / (EPS * absum)
        assert errR.max() <= sum_roundings(S), (A, S, errR.max())
        yd, vd, lam, trace, ref = pr.direct(xs, S, iters)
        assert np.array_equal(st["ref"], ref) and not st["flags"].any()
        for i in range(n):
            err, bound = np.linalg.norm(v[i].astype(np.complex128) - vd[i]), weight_bound(X[i], iters, S)
            assert err <= bound, (A, S, iters, err, bound)
            if report is not None:
                rv = report.setdefault("v", {})
                rv[A, S, iters] = max(rv.get((A, S, iters), 0.0), err / bound)
        v64 = v.astype(np.complex128)
        want = np.einsum("na,nas->ns", v64.conj(), X)
        l1 = lambda z: np.abs(z.real) + np.abs(z.imag)
        terms = np.einsum("na,nas->ns", l1(v64), l1(X))
        erry = np.maximum(np.abs(y.real - want.real), np.abs(y.imag - want.imag)) / (EPS * terms)
        assert erry.max() <= 2 * A, (A, S, erry.max())
        assert np.allclose(st["lambda"], lam, rtol=1e-4) and np.allclose(st["trace"], trace, rtol=1e-5)
        if report is not None:
            report.setdefault("R", {})[A, S] = (float(errR.max()), sum_roundings(S))
            report.setdefault("y", {})[A, S] = (float(erry.max()), 2 * A)


def _tile_of_equal_samples():
    """one sample whose |x|^2 cannot be added 64 times left to right without a rounding, found without the reference"""
    rng = np.random.default_rng(5)
    while True:
        x = np.complex64(complex(rng.uniform(1, 2), rng.uniform(1, 2)))
        p = fma32(x.imag, x.imag, fma32(x.real, x.real, F32(0)))[()]
        acc = p
        for _ in range(63):
            acc = F32(acc + p)
        if acc != F32(64) * p:
            return x, p


def check_equal_lanes_sum_exactly(mutant=None):
    """64 equal samples: the butterfly only ever adds equal values, so the fold is 64 |x|^2 exactly and, with two identical
    antennas, the trace is 128 |x|^2 exactly; a left-to-right sum rounds on the way (rule 24's argument, across the lanes)"""
    x, p = _tile_of_equal_samples()
    xs = [np.full((1, 64), x, np.complex64)] * 2
    _, v, st = pr.combine(xs, 64, 0, mutant=mutant)
    assert st["trace"][0] == F32(128) * p and st["flags"][0] == 0
    Rre, _ = pr.covariance(xs, 64, mutant)
    assert (Rre[0] == F32(64) * p).all()


def check_reference_antenna_is_the_strongest(mutant=None):
    """item 2: the greatest R_aa; a tie keeps the lower index; the output phase is that antenna's"""
    for A in (2, 4, 8):
        xs = rows.build("known_gain", A, 128, 2)
        _, r = rows.known_gain_weights(A)
        y, v, st = pr.combine(xs, 128, 1, mutant=mutant)
        assert (st["ref"] == r).all() and (v[:, r].imag == 0).all() and (v[:, r].real > 0).all()
    for A in (2, 3, 8):
        xs = rows.build("tie", A, 128, 37)
        _, v, st = pr.combine(xs, 128, 0, mutant=mutant)
        assert (st["ref"] == max(A - 2, 0)).all()


def check_output_snr_is_the_sum_of_the_antennas(mutant=None, report=None):
    """A frame-sized row through A known flat gains, equal noise: the weights align with the gains and the output SNR is the
    sum of the antennas' SNRs.  The signal part of the stream is its projection on the transmitted row, the rest is noise.
    Tolerance: the blind eigenvector of S samples misses the gains by about (A - 1) / (S SNR_sum) in power, and
    the A noise rows are only orthogonal to about sqrt(A / S): the ratio is asserted within 4 sqrt(A / S) (four sigma)."""
    S, n = 4096, 4
    for A, snr_each in ((2, 2.0), (4, 1.0), (8, 0.5)):
        rng = np.random.default_rng(40 + A)
        s = rows.noise(rng, (n, S))
        g = rows.noise(rng, (n, A, 1)).astype(np.complex128)
        g *= np.sqrt(snr_each * A) / np.linalg.norm(g, axis=1, keepdims=True)       # mean SNR per antenna snr_each, noise power 1
        nz = [rows.noise(rng, (n, S)) for _ in range(A)]
        xs = [(g[:, a] * s + nz[a]).astype(np.complex64) for a in range(A)]
        y, v, st = pr.combine(xs, S, 2, mutant=mutant)
        v64, y64, s64 = v.astype(np.complex128), y.astype(np.complex128), s.astype(np.complex128)
        alpha = (y64 * s64.conj()).sum(axis=1) / (np.abs(s64) ** 2).sum(axis=1)        # the stream's own signal part: its projection on s
        sig = alpha[:, None] * s64
        snr_out = (np.abs(sig) ** 2).sum(axis=1) / (np.abs(y64 - sig) ** 2).sum(axis=1)
        snr_sum = sum((np.abs(g[:, a] * s) ** 2).sum(axis=1) / (np.abs(nz[a]) ** 2).sum(axis=1) for a in range(A))
        align = np.abs(np.einsum("na,na->n", v64.conj(), g[:, :, 0])) / np.linalg.norm(g[:, :, 0], axis=1)
        tol = 4 * np.sqrt(A / S)
        assert (align ** 2 >= 1 - tol).all(), (A, align)
        assert (np.abs(snr_out / snr_sum - 1) <= tol).all(), (A, snr_out / snr_sum)
        if report is not None:
            report[A] = (float(np.abs(snr_out / snr_sum - 1).max()), float(tol))


def check_weights_have_unit_norm(mutant=None):
    """item 3: the noise power of the stream is one antenna's; known gains come back as g / |g| within weight_bound"""
    for A in (2, 3, 8):
        for iters in (0, 2, 4):
            S = 320
            xs = rows.build("known_gain", A, S, 2)
            _, v, st = pr.combine(xs, S, iters, mutant=mutant)
            want, _ = rows.known_gain_weights(A)
            X = np.stack([x.astype(np.complex128) for x in xs], axis=1)
            for i in range(2):
                assert abs(np.linalg.norm(v[i].astype(np.complex128)) - 1) <= (2 * A + 4) * EPS
                assert np.linalg.norm(v[i] - want) <= weight_bound(X[i], iters, S), (A, iters)
            # rank one: lambda = trace
            assert np.allclose(st["lambda"], st["trace"], rtol=1e-5)


def check_reference_weight_is_real_and_nonnegative(mutant=None):
    """item 3's rotation: after a power iteration v_r carries a rounding-sized imaginary part; the rule removes it exactly, so
    the output phase is antenna r's"""
    xs = rows.build("scene", 4, 320, 16, seed=3)
    _, v, st = pr.combine(xs, 320, 3, mutant=mutant)
    vr = v[np.arange(16), st["ref"]]
    assert (vr.imag == 0).all() and not np.signbit(vr.imag).any() and (vr.real > 0).all()


CHECKS = {"lane_sum": check_equal_lanes_sum_exactly, "ref0": check_reference_antenna_is_the_strongest,
          "noconj": check_output_snr_is_the_sum_of_the_antennas, "nonorm": check_weights_have_unit_norm,
          "norot": check_reference_weight_is_real_and_nonnegative}


def test_against_float64():
    check_against_float64()


def test_equal_lanes_sum_exactly():
    check_equal_lanes_sum_exactly()


def test_reference_antenna_is_the_strongest():
    check_reference_antenna_is_the_strongest()


def test_output_snr_is_the_sum_of_the_antennas():
    check_output_snr_is_the_sum_of_the_antennas()


def test_weights_have_unit_norm():
    check_weights_have_unit_norm()


def test_reference_weight_is_real_and_nonnegative():
    check_reference_weight_is_real_and_nonnegative()


# ---- item 5 and the exact clauses ----------------------------------------------------------------------------------------------

def test_one_antenna_is_a_copy():
    for case in ("scene", "nan_first", "inf", "zero_slot"):
        xs = rows.build(case, 1, 128, 3)
        y, v, st = pr.combine(xs, 128, 2)
        assert rows.same_bits(y, xs[0]) and (v == 1).all() and rows.same_bits(st, np.zeros(3, pr.STATS_DTYPE))


@pytest.mark.parametrize("A", (2, 3, 8))
def test_degenerate_slots_copy_antenna_0(A):
    """a trace that is not finite or not > 0: y = x_0 bit for bit, v = e_0, the flag; the other slots are combined"""
    for case, bad in (("zero_slot", [0]), ("nan_first", [0]), ("nan_later", [0]), ("inf", [0, 3])):
        xs = rows.build(case, A, 128, 4)
        y, v, st = pr.combine(xs, 128, 2)
        for i in range(4):
            if i in bad:
                assert st["flags"][i] == pr.DEGENERATE and st["ref"][i] == 0 and st["lambda"][i] == 0
                assert rows.same_bits(y[i], xs[0][i]) and v[i, 0] == 1 and (v[i, 1:] == 0).all()
            else:
                assert st["flags"][i] == 0 and np.isfinite(y[i]).all() and abs(np.linalg.norm(v[i]) - 1) < 1e-5
    xs = rows.build("zero_slot", A, 128, 2)
    assert pr.combine(xs, 128, 0)[2]["trace"][0] == 0


def test_an_overflowing_norm_is_degenerate():
    """the squares of the covariance column leave float32: the normalisation is not finite, the slot falls back"""
    xs = [x * F32(1e9) for x in rows.build("scene", 2, 64, 1)]
    y, v, st = pr.combine(xs, 64, 1)
    assert np.isfinite(st["trace"][0]) and st["flags"][0] == pr.DEGENERATE and rows.same_bits(y, xs[0])


@pytest.mark.parametrize("A", (2, 4, 8))
def test_identical_antennas_get_equal_weights(A):
    xs = rows.build("identical", A, 320, 2)
    y, v, st = pr.combine(xs, 320, 2)
    assert (st["ref"] == 0).all() and np.allclose(v, 1 / np.sqrt(A), atol=1e-6)
    assert np.allclose(y, np.sqrt(A) * xs[0], rtol=1e-5, atol=1e-6)


def test_an_all_zero_antenna_gets_no_weight():
    xs = rows.build("zero_antenna", 3, 320, 2)
    y, v, st = pr.combine(xs, 320, 2)
    assert (v[:, 1] == 0).all() and not st["flags"].any()
    y2, v2, _ = pr.combine([xs[0], xs[2]], 320, 2)
    assert rows.same_bits(v[:, [0, 2]], v2) and rows.same_bits(y, y2)


def test_the_order_does_not_depend_on_the_batch():
    """slot i of a batch is the slot alone: nothing depends on n_slots or on where the slot lies"""
    xs = rows.build("scene", 3, 320, 5)
    y, v, st = pr.combine(xs, 320, 2)
    y1, v1, st1 = pr.combine([x[3:4] for x in xs], 320, 2)
    assert rows.same_bits(y[3:4], y1) and rows.same_bits(v[3:4], v1) and rows.same_bits(st[3:4], st1)


@pytest.mark.parametrize("mutant", pr.MUTANTS)
def test_every_mutant_is_caught_by_its_named_test(mutant):
    CHECKS[mutant]()                                    # the rule passes ...
    with pytest.raises(AssertionError):                 # ... and the mutant does not
        CHECKS[mutant](mutant)


def mutation_record() -> str:
    lines = ["Mutants of tests/precombine_ref.py (NUMERICS.md rule 33) and the tests of tests/test_precombine_ref.py that fail when the",
             "reference is run with them (x = fails, . = passes).  Asserted: every mutant fails the test named for it",
             "(test_every_mutant_is_caught_by_its_named_test).", ""]
    names = list(CHECKS.values()) + [check_against_float64]
    for i, c in enumerate(names):
        lines.append("  T%d = test_%s" % (i + 1, c.__name__[len("check_"):]))
    lines += ["", "%-10s %s   named test" % ("mutant", " ".join("T%d" % (i + 1) for i in range(len(names))))]
    for m in pr.MUTANTS:
        marks = []
        for c in names:
            try:
                c(m)
                marks.append(". ")
            except AssertionError:
                marks.append("x ")
        lines.append("%-10s %s   T%d" % (m, " ".join(marks), names.index(CHECKS[m]) + 1))
    rep = {}
    check_against_float64(report=rep)
    lines += ["", "test_against_float64, the rule itself (scene rows of tests/precombine_rows.py; antennas, slot_len[, iters]):",
              "  largest error of a component of R in units of 2^-24 sum |terms| (bound: 2 ceil(tiles / 4) + 8)"]
    lines += ["    A = %d, S = %d: %.2f (bound %d)" % (k + v) for k, v in sorted(rep["R"].items())]
    lines += ["  largest error of a component of y in units of 2^-24 sum |terms| (bound: 2 A)"]
    lines += ["    A = %d, S = %d: %.2f (bound %d)" % (k + v) for k, v in sorted(rep["y"].items())]
    lines += ["  largest || v32 - v64 || as a fraction of weight_bound()"]
    lines += ["    A = %d, S = %d, iters = %d: %.4f" % (k + (v,)) for k, v in sorted(rep["v"].items())]
    snr = {}
    check_output_snr_is_the_sum_of_the_antennas(report=snr)
    lines += ["", "test_output_snr_is_the_sum_of_the_antennas: largest |SNR_out / sum SNR_a - 1| (tolerance 4 sqrt(A / S))"]
    lines += ["    A = %d: %.4f (%.4f)" % ((k,) + v) for k, v in sorted(snr.items())]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    open(os.path.join(ROOT, "profiles", "precombine_mutations.txt"), "w").write(mutation_record())
