"""NUMERICS.md rule 31 on the host: tests/irs_optimize_w_ref.py, the restatement of wifirx_irs_optimize_weighted, against
  * the three properties that hold exactly (every weight 1.0f: rule 30 bit for bit, a NaN staying a NaN; every weight 2^k: rule
    30's codes and sweeps and 2^k times its power; rows of weight zero: the same bits whatever they hold, as with those rows
    zeroed, and as with fewer rows when they are the last ones), early exit = the full run, and the all-zero weight vector;
  * the float64 definition, for signed weights: every single decision within the rule's allowance of the best one (a float64
    shadow of the float32 run), the objective of the final codes not below the start's by more than the allowance per update, the
    power values within the rule's bound of the definition under the same codes, and `direct()`, the same ascent in float64,
    within the bound wherever it ends at the same codes (the distances are printed and kept as profiles/irs_optimize_w_tests.txt);
  * the operating point (tests/irs_optimize_w_point.py, profiles/irs_optimize_w_operating_point.json): the file holds what the
    script recomputes; the one inequality asserted is the objective's invariant at sigma = 0, the ratios are recorded;
  * six mutants of the restatement, each caught by the check named for it (test_mutation_table prints the log kept as
    profiles/irs_optimize_w_mutations.txt).
Every mutation check is a function check_*(mutant=None) that raises AssertionError."""
import json
import math
import os

import numpy as np
import pytest

import irs_optimize_ref as orf
import irs_optimize_w_point as wp
import irs_optimize_w_ref as wrf
from wifirx import irs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 4), (17, 9), (64, 7), (65, 8), (128, 9), (40, 33), (5, 64)]     # (R, G)
STARTS = (wrf.START_REF, wrf.START_GIVEN, wrf.START_ZERO)
KEYS = ("codes", "psi", "power", "sweeps")


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def cases():
    """(q [2, R, J], w [R], bits, start, blocked, codes_in) over the shapes: signed weights, about a tenth of them zero"""
    rng = np.random.default_rng(31)
    out = []
    for i, (R, G) in enumerate(SHAPES):
        for j in range(3):
            bits, start, blocked = 1 + (i + j) % 3, STARTS[j], bool((i + j) & 1)
            w = rng.standard_normal(R).astype(np.float32)
            w[rng.random(R) < 0.1] = 0
            out.append((crandn(rng, 2, R, G + 1), w, bits, start, blocked, rng.integers(0, 1 << bits, (2, G)).astype(np.uint8)))
    return out


CASES = cases()


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in KEYS)


# ---- the properties that hold exactly ----

def test_no_weights_is_the_unweighted_restatement_itself():
    q = crandn(np.random.default_rng(1), 2, 3, 5)
    assert same(wrf.optimize(q, 2, 3), orf.optimize(q, 2, 3))
    assert wrf.fold is orf.fold and wrf.argmax is orf.argmax and wrf.start_codes is orf.start_codes      # imported, not copied


def test_unit_weights_are_rule_30_bit_for_bit():
    for q, _, bits, start, blocked, ci in CASES:
        one = np.ones(q.shape[1], np.float32)
        assert same(wrf.optimize(q, bits, 4, start, blocked, ci, weights=one), orf.optimize(q, bits, 4, start, blocked, ci))
    q = crandn(np.random.default_rng(2), 1, 70, 6)
    q[0, 66, 3] = np.nan                                           # a NaN stays a NaN
    a, b = wrf.optimize(q, 2, 2, weights=np.ones(70, np.float32)), orf.optimize(q, 2, 2)
    assert np.isnan(a["power"]).all() and np.isnan(b["power"]).all() and a["codes"].tobytes() == b["codes"].tobytes()


@pytest.mark.parametrize("k", [2, -3, 40])
def test_a_power_of_two_scales_the_power_alone(k):
    for q, _, bits, start, blocked, ci in CASES:
        a = orf.optimize(q, bits, 4, start, blocked, ci)
        b = wrf.optimize(q, bits, 4, start, blocked, ci, weights=np.full(q.shape[1], 2.0 ** k, np.float32))
        assert a["codes"].tobytes() == b["codes"].tobytes() and a["sweeps"].tobytes() == b["sweeps"].tobytes()
        assert (np.float32(2.0 ** k) * a["power"]).tobytes() == b["power"].tobytes()


def check_zero_weight_rows_are_absent(mutant=None):
    """rows of weight zero (either sign) holding NaN, infinities and large values, on both sides of row 64: the bits of the call
    with those rows zeroed, and, when they are the last rows, of the call with fewer rows"""
    rng = np.random.default_rng(3)
    for R, dead, start in ((70, (3, 40, 66, 69), wrf.START_ZERO), (128, (1, 63, 64, 127), wrf.START_REF), (9, (5,), wrf.START_GIVEN)):
        q, w = crandn(rng, 2, R, 12), rng.standard_normal(R).astype(np.float32)
        ci = rng.integers(0, 4, (2, 11)).astype(np.uint8)
        w[list(dead)] = [0.0, -0.0, 0.0, -0.0][:len(dead)]
        bad, zeroed = q.copy(), q.copy()
        bad[:, list(dead)] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e38], np.float32), (2, len(dead), 12))
        zeroed[:, list(dead)] = 0
        a = wrf.optimize(bad, 2, 4, start, codes_in=ci, weights=w, mutant=mutant)
        assert same(a, wrf.optimize(zeroed, 2, 4, start, codes_in=ci, weights=w)) and np.isfinite(a["power"]).all(), R
    for R, keep in ((70, 64), (70, 66), (128, 5), (64, 63)):
        q, w = crandn(rng, 2, R, 10), rng.standard_normal(R).astype(np.float32)
        w[keep:] = 0
        q[:, keep:] = np.nan
        assert same(wrf.optimize(q, 2, 4, weights=w, mutant=mutant), wrf.optimize(q[:, :keep], 2, 4, weights=w[:keep])), (R, keep)


def test_zero_weight_rows_are_absent():
    check_zero_weight_rows_are_absent()


def test_all_zero_weights_turn_every_code_to_0_and_stop():
    """z = +0 at every step: the argmax takes c = 0 on the tie, so sweep 1 turns every code to 0 and sweep 2 changes nothing"""
    rng = np.random.default_rng(4)
    q, ci = crandn(rng, 3, 66, 8), rng.integers(1, 4, (3, 7)).astype(np.uint8)
    got = wrf.optimize(q, 2, 6, wrf.START_GIVEN, codes_in=ci, weights=np.zeros(66, np.float32))
    assert not got["codes"].any() and got["power"].tobytes() == bytes(got["power"].nbytes) and (got["sweeps"] == 1).all()
    got = wrf.optimize(q, 2, 6, wrf.START_ZERO, weights=np.zeros(66, np.float32))
    assert not got["codes"].any() and not got["sweeps"].any()


def test_early_exit_equals_the_full_run():
    stopped = 0
    for q, w, bits, start, blocked, ci in CASES:
        for r in range(2):
            six = wrf.optimize_set(q[r], w, bits, 6, start, blocked, ci[r])
            nine = wrf.optimize_set(q[r], w, bits, 9, start, blocked, ci[r])
            full = wrf.optimize_set(q[r], w, bits, 9, start, blocked, ci[r], early_exit=False)
            assert nine[0].tobytes() == full[0].tobytes() and nine[1].tobytes() == full[1].tobytes() and nine[2] == full[2]
            assert six[1].tobytes() == nine[1][:7].tobytes()
            if nine[2] < 6:
                assert six[0].tobytes() == nine[0].tobytes() and six[2] == nine[2]
                assert (nine[1][nine[2]:] == nine[1][-1]).all()
                stopped += 1
    assert stopped >= len(CASES)                                   # the early exit was in fact taken on most sets


# ---- against the float64 definition ----

def shadow(q, w, bits, max_sweeps, start, blocked, ci):
    """the float32 run of one set with every decision judged in float64: returns (result, worst loss against the best code of a
    step, number of updates, float64 objective of the start codes, of the final codes)"""
    trace = []
    res = wrf.optimize_set(q, w, bits, max_sweeps, start, blocked, ci, trace=trace)
    wd, qd = wrf.used(w, np.asarray(q, np.complex128))
    ph = irs.PHASES.astype(np.complex128)
    up = 3 - bits
    codes = wrf.start_codes(np.asarray(q, np.complex64), bits, start, blocked, ci).copy()
    p_start = wrf.true_power(q, w, codes, bits, blocked)
    d = 0 if blocked else qd[:, 0]
    worst, updates = 0.0, 0
    for g, c_old, c_new in trace:
        assert codes[g] == c_old
        s = d + (qd[:, 1:] * ph[codes.astype(np.intp) << up][None, :]).sum(axis=1)
        z = (wd * np.conj(s - qd[:, g + 1] * ph[c_old << up]) * qd[:, g + 1]).sum()
        m = (z * ph[np.arange(1 << bits) << up]).real
        worst = max(worst, 2 * (m.max() - m[c_new]))              # P_w = const + 2 Re(z C_c)
        updates += c_new != c_old
        codes[g] = c_new
    assert codes.tobytes() == res[0].tobytes()
    return res, worst, updates, p_start, wrf.true_power(q, w, codes, bits, blocked)


def test_ascent_against_the_float64_definition():
    """signed weights: every decision within the allowance of the best one; the objective of the final codes not below the
    start's by more than the allowance per update; the float32 power within the rule's bound of the definition"""
    lines = []
    for q, w, bits, start, blocked, ci in CASES:
        for r in range(2):
            (codes, power, sweeps), worst, updates, p_start, p_final = shadow(q[r], w, bits, 4, start, blocked, ci[r])
            allow, pb = wrf.decision_allowance(q[r], w, 4, blocked), wrf.power_bound(q[r], w, 4, blocked)
            assert worst <= allow
            assert p_final >= p_start - updates * allow
            assert abs(float(power[0]) - p_start) <= pb and abs(float(power[-1]) - p_final) <= pb
            if allow > 0:
                lines.append((q.shape[1], q.shape[2] - 1, bits, worst / allow, abs(float(power[-1]) - p_final) / pb, p_start < 0))
    assert any(l[5] for l in lines)                                # a negative objective is among the cases
    print("\nR, G, bits: worst loss of a decision / allowance, |power - P_w| / bound")
    for l in lines[::2]:
        print("%3d %3d %d: %.3g  %.3g%s" % (l[:5] + ("  (P_w < 0)" if l[5] else "",)))


def test_direct_float64_ascent_by_power():
    """direct() against the float32 rule: the same codes on nearly every set, and then the same power within the rule's bound.  A
    near tie may send the two runs to different codes; those sets are counted, not bounded"""
    equal, differ, dist = 0, 0, 0.0
    for q, w, bits, start, blocked, ci in CASES:
        for r in range(2):
            c32, p32, _ = wrf.optimize_set(q[r], w, bits, 4, start, blocked, ci[r])
            c64, p64, _ = wrf.direct(q[r], w, bits, 4, start, blocked, ci[r])
            if c32.tobytes() == c64.tobytes():
                equal += 1
                pb = wrf.power_bound(q[r], w, 4, blocked)
                assert (np.abs(p32.astype(np.float64) - p64) <= pb).all()
                if pb > 0:
                    dist = max(dist, float(np.abs(p32.astype(np.float64) - p64).max() / pb))
            else:
                differ += 1
    print("\ndirect(): %d sets with the float32 rule's codes (largest |power32 - power64| / bound %.3g), %d sets with other codes"
          % (equal, dist, differ))
    assert equal >= 0.9 * (equal + differ)


# ---- the operating point ----

@pytest.fixture(scope="module")
def points():
    return [wp.point(name, s) for name in wp.SCENES for s in wp.sigmas()]


def test_operating_point_file_is_what_the_script_computes(points):
    with open(os.path.join(ROOT, "profiles", "irs_optimize_w_operating_point.json")) as f:
        kept = json.load(f)
    now = json.loads(json.dumps(wp.document([wp.record(pt) for pt in points])))

    def equal(a, b, where):
        """the same document; a float to 1e-9 of its value (the float64 sums and transforms behind the figures may round in another
        order on another host, which moves them by parts in 1e15, not in 1e9)"""
        if isinstance(a, dict):
            assert isinstance(b, dict) and list(a) == list(b), where
            for k in a:
                equal(a[k], b[k], where + (k,))
        elif isinstance(a, list):
            assert isinstance(b, list) and len(a) == len(b), where
            for i, (x, y) in enumerate(zip(a, b)):
                equal(x, y, where + (i,))
        elif isinstance(a, float):
            assert isinstance(b, float) and abs(a - b) <= 1e-9 * abs(a), (where, a, b)
        else:
            assert a == b, (where, a, b)

    equal(kept, now, ())


def test_weighted_objective_does_not_fall_at_sigma_0(points):
    """the one inequality: per set, the float64 weighted objective (of the coefficients the optimiser was given) under the
    weighted codes is not below that under the start codes by more than the allowance per update.  The ratios are recorded."""
    for pt in points:
        if pt["sigma"] != 0.0:
            continue
        G = pt["est"].shape[2] - 1
        for k, w in pt["weights"].items():
            for r in range(wp.SETS):
                allow = wrf.decision_allowance(pt["est"][r], w, wp.SWEEPS, True) * G * wp.SWEEPS
                after = wrf.true_power(pt["est"][r], w, pt["res"][k]["codes"][r], wp.BITS, True)
                before = wrf.true_power(pt["est"][r], w, pt["ref_codes"][r], wp.BITS, True)
                assert after >= before - allow, (pt["scene"], k, r)


# ---- the mutants ----

def one(q, w, bits, start=wrf.START_ZERO, blocked=False, ci=None, mutant=None, sweeps=2):
    return wrf.optimize_set(np.asarray(q, np.complex64), np.asarray(w, np.float32), bits, sweeps, start, blocked, ci, mutant)


def check_weights_reach_z(mutant=None):
    """rows (d, e) = (1, -1.2) and (1, 2) with w = (1, 0.1): z = -1.2 + 0.2 < 0 turns the code to 1; unweighted z = +0.8 keeps 0"""
    codes, power, _ = one([[1, -1.2], [1, 2]], [1, 0.1], 1, mutant=mutant)
    assert codes.tolist() == [1] and abs(power[-1] - (4.84 + 0.1)) < 1e-5


def check_sign_of_a_weight(mutant=None):
    """one row (1, 1) with w = -1: z = -1, the code turns to 1 and P_w rises from -4 to 0; with |w| it stays"""
    codes, power, _ = one([[1, 1]], [-1], 1, mutant=mutant)
    assert codes.tolist() == [1] and power.tolist() == [-4, 0, 0]


def check_power_is_weighted(mutant=None):
    codes, power, _ = one([[1, 1], [2, 1]], [0.5, -0.25], 1, mutant=mutant)
    assert codes.tolist() == [0] and power.tolist() == [2 - 2.25] * 3


def check_rows_above_64_read_their_own_weight(mutant=None):
    """row 0 = (1, 1) with w_0 = 0.25, row 64 = (1, -3) with w_64 = 1: z = 0.25 - 3 turns the code and the power is
    0.25 x 0 + 1 x 16; with row 0's weight on row 64 the code turns too (z = 0.25 - 0.75), but the power is 0.25 x 16"""
    q, w = np.zeros((65, 2), np.complex64), np.zeros(65, np.float32)
    q[0], q[64], w[0], w[64] = (1, 1), (1, -3), 0.25, 1
    codes, power, _ = one(q, w, 1, mutant=mutant)
    assert codes.tolist() == [1] and power.tolist() == [0.25 * 4 + 4, 16, 16]


def check_sets_read_their_own_block(mutant=None):
    q = np.array([[[1, 1]], [[1, 1]]], np.complex64)
    got = wrf.optimize(q, 1, 2, wrf.START_ZERO, weights=np.array([[1], [-1]], np.float32), mutant=mutant)
    assert got["codes"].tolist() == [[0], [1]] and got["power"].tolist() == [[4, 4, 4], [-4, 0, 0]]


CHECKS = {"dropped": check_weights_reach_z, "abs": check_sign_of_a_weight, "power": check_power_is_weighted,
          "zero_kept": check_zero_weight_rows_are_absent, "upper": check_rows_above_64_read_their_own_weight,
          "sets": check_sets_read_their_own_block}


@pytest.mark.parametrize("name", wrf.MUTANTS)
def test_check_passes_on_the_restatement(name):
    CHECKS[name]()


@pytest.mark.parametrize("name", wrf.MUTANTS)
def test_mutant_fails_the_check_named_for_it(name):
    with pytest.raises(AssertionError):
        CHECKS[name](name)


def test_mutation_table():
    """every check on the restatement and on every mutant: the check named for a mutant fails on it (the table that
    `pytest tests/test_irs_optimize_w_ref.py -k mutation_table -s` prints is kept as profiles/irs_optimize_w_mutations.txt)"""
    lines = ["mutant      " + "".join("%-44s" % f.__name__ for f in CHECKS.values())]
    for m in (None,) + wrf.MUTANTS:
        row = []
        for name, f in CHECKS.items():
            try:
                f(m)
                row.append("pass")
            except AssertionError:
                row.append("FAIL")
            if m is None or name == m:
                assert row[-1] == ("pass" if m is None else "FAIL"), (m, name)
        lines.append("%-12s" % (m or "(none)") + "".join("%-44s" % r for r in row))
    print("\n" + "\n".join(lines))
