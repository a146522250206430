"""NUMERICS.md rule 30 on the host: tests/irs_optimize_ref.py, the restatement of wifirx_irs_optimize, against
  * the four properties that hold exactly (scaling by 4, all-zero extra rows, rows copied into the upper lanes' half, no sweep =
    rule 29's decision), and early exit = the full run;
  * the float64 definition: the power of the final codes is not below that of the start codes, no power trace falls, every
    single decision is within the rule's allowance of the best one (a float64 shadow of the float32 run), the power values are
    within the rule's bound of the definition under the same codes, and `direct()`, the same ascent in float64, ends at the same
    power wherever it ends at the same codes (near ties may send the two to different codes; the distances are printed and kept
    as profiles/irs_optimize_tests.txt);
  * the operating point (tests/irs_optimize_point.py, profiles/irs_optimize_operating_point.json): the joint decision collects
    more power than rule 29's on every scene;
  * six mutants of the restatement, each caught by the check named for it (test_mutation_table prints the log kept as
    profiles/irs_optimize_mutations.txt).
Every mutation check is a function check_*(mutant=None) that raises AssertionError."""
import math

import numpy as np
import pytest

import irs_estimate_ref as er
import irs_optimize_point as op
import irs_optimize_ref as orf
from wifirx import irs

SHAPES = [(1, 1), (3, 4), (17, 9), (64, 7), (65, 8), (128, 9), (40, 33), (5, 64)]     # (R, G)
STARTS = (orf.START_REF, orf.START_GIVEN, orf.START_ZERO)


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def cases():
    """(q [2, R, J], bits, start, blocked, codes_in) over the shapes: every bits, start and blocked at least once per shape pair"""
    rng = np.random.default_rng(30)
    out = []
    for i, (R, G) in enumerate(SHAPES):
        for j in range(3):
            bits, start, blocked = 1 + (i + j) % 3, STARTS[j], bool((i + j) & 1)
            out.append((crandn(rng, 2, R, G + 1), bits, start, blocked, rng.integers(0, 1 << bits, (2, G)).astype(np.uint8)))
    return out


CASES = cases()


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("codes", "psi", "power", "sweeps"))


# ---- the properties that hold exactly ----

def test_scaling_by_4_scales_the_power_by_16():
    for q, bits, start, blocked, ci in CASES:
        a, b = orf.optimize(q, bits, 4, start, blocked, ci), orf.optimize(4 * q, bits, 4, start, blocked, ci)
        assert a["codes"].tobytes() == b["codes"].tobytes() and a["sweeps"].tobytes() == b["sweeps"].tobytes()
        assert (16 * a["power"]).tobytes() == b["power"].tobytes()


def test_all_zero_extra_rows_change_no_bit():
    for q, bits, start, blocked, ci in CASES:
        R = q.shape[1]
        if R == 128:
            continue
        for extra in sorted({1, 64 - R if R < 64 else 1, 128 - R}):
            wide = np.concatenate([q, np.zeros((2, extra, q.shape[2]), np.complex64)], axis=1)
            assert same(orf.optimize(q, bits, 4, start, blocked, ci), orf.optimize(wide, bits, 4, start, blocked, ci)), (R, extra)


def test_rows_copied_into_the_upper_half_double_the_power():
    for q, bits, start, blocked, ci in CASES:
        R = q.shape[1]
        if R > 64:
            continue
        two = np.zeros((2, 64 + R, q.shape[2]), np.complex64)
        two[:, :R], two[:, 64:] = q, q
        a, b = orf.optimize(q, bits, 4, start, blocked, ci), orf.optimize(two, bits, 4, start, blocked, ci)
        assert a["codes"].tobytes() == b["codes"].tobytes() and (2 * a["power"]).tobytes() == b["power"].tobytes()


@pytest.mark.parametrize("blocked", [False, True])
def test_no_sweep_from_the_reference_start_is_rule_29_s_decision(blocked):
    rng = np.random.default_rng(29)
    for bits in (1, 2, 3):
        est = crandn(rng, 5, 6, 17)
        est[1, 0, 0] = 0                                           # a zero direct estimate: the real axis
        got = orf.optimize(est, bits, 0, orf.START_REF, blocked)
        assert got["codes"].tobytes() == er.decide(est, bits, blocked=blocked).tobytes()
        assert got["sweeps"].tobytes() == bytes(5) and got["power"].shape == (5, 1)


def test_early_exit_equals_the_full_run():
    stopped = 0
    for q, bits, start, blocked, ci in CASES:
        for r in range(2):
            six = orf.optimize_set(q[r], bits, 6, start, blocked, ci[r])
            nine = orf.optimize_set(q[r], bits, 9, start, blocked, ci[r])
            full = orf.optimize_set(q[r], bits, 9, start, blocked, ci[r], early_exit=False)
            assert nine[0].tobytes() == full[0].tobytes() and nine[1].tobytes() == full[1].tobytes() and nine[2] == full[2]
            assert six[1].tobytes() == nine[1][:7].tobytes()
            if nine[2] < 6:                                        # ended before the sixth sweep: the three are one run
                assert six[0].tobytes() == nine[0].tobytes() and six[2] == nine[2]
                assert (nine[1][nine[2]:] == nine[1][-1]).all()
                stopped += 1
    assert stopped >= len(CASES)                                   # the early exit was in fact taken on most sets


# ---- against the float64 definition ----

def shadow(q, bits, max_sweeps, start, blocked, ci):
    """the float32 run of one set with every decision judged in float64: returns (result, worst loss against the best code of a
    step, number of updates, float64 power of the start codes, of the final codes)"""
    trace = []
    res = orf.optimize_set(q, bits, max_sweeps, start, blocked, ci, trace=trace)
    qd = np.asarray(q, np.complex128)
    ph = irs.PHASES.astype(np.complex128)
    up = 3 - bits
    codes = orf.start_codes(np.asarray(q, np.complex64), bits, start, blocked, ci).copy()
    p_start = orf.true_power(qd, codes, bits, blocked)[0]
    d = 0 if blocked else qd[:, 0]
    worst, updates = 0.0, 0
    for g, c_old, c_new in trace:
        assert codes[g] == c_old
        s = d + (qd[:, 1:] * ph[codes.astype(np.intp) << up][None, :]).sum(axis=1)
        z = (np.conj(s - qd[:, g + 1] * ph[c_old << up]) * qd[:, g + 1]).sum()
        m = (z * ph[np.arange(1 << bits) << up]).real
        worst = max(worst, 2 * (m.max() - m[c_new]))              # P = const + 2 Re(z C_c)
        updates += c_new != c_old
        codes[g] = c_new
    assert codes.tobytes() == res[0].tobytes()
    return res, worst, updates, p_start, orf.true_power(qd, codes, bits, blocked)[0]


def test_ascent_against_the_float64_definition():
    """every decision within the allowance of the best one; the final power not below the start's; no trace falls; the float32
    power within the rule's bound of the definition under the same codes"""
    lines = []
    for q, bits, start, blocked, ci in CASES:
        for r in range(2):
            (codes, power, sweeps), worst, updates, p_start, p_final = shadow(q[r], bits, 4, start, blocked, ci[r])
            allow, pb = orf.decision_allowance(q[r], 4, blocked), orf.power_bound(q[r], 4, blocked)
            G = q.shape[2] - 1
            lines.append((q.shape[1], G, bits, worst / allow, abs(float(power[-1]) - p_final) / pb))
            assert worst <= allow
            assert p_final >= p_start - updates * allow
            assert (np.diff(power.astype(np.float64)) >= -(G * allow + 2 * pb)).all()
            assert abs(float(power[0]) - p_start) <= pb and abs(float(power[-1]) - p_final) <= pb
    print("\nR, G, bits: worst loss of a decision / allowance, |power - P| / bound")
    for l in lines[::2]:
        print("%3d %3d %d: %.3g  %.3g" % l)


def test_direct_float64_ascent_by_power():
    """direct() against the float32 rule: the same codes on nearly every set, and then the same power within the rule's bound.  A
    near tie may send the two runs to different codes; those sets are counted and their power distance printed, not bounded."""
    equal, differ, dist, far = 0, 0, 0.0, 0.0
    for q, bits, start, blocked, ci in CASES:
        for r in range(2):
            c32, p32, _ = orf.optimize_set(q[r], bits, 4, start, blocked, ci[r])
            c64, p64, _ = orf.direct(q[r], bits, 4, start, blocked, ci[r])
            if c32.tobytes() == c64.tobytes():
                equal += 1
                pb = orf.power_bound(q[r], 4, blocked)
                assert (np.abs(p32.astype(np.float64) - p64) <= pb).all()
                dist = max(dist, float(np.abs(p32.astype(np.float64) - p64).max() / pb))
            else:
                differ += 1
                far = max(far, abs(float(p32[-1]) - p64[-1]) / p64[-1])
    print("\ndirect(): %d sets with the float32 rule's codes (largest |power32 - power64| / bound %.3g), %d sets with other codes "
          "(largest relative power distance %.3g)" % (equal, dist, differ, far))
    assert equal >= 0.9 * (equal + differ)


# ---- the operating point ----

@pytest.fixture(scope="module")
def points():
    return [op.point(name, s) for name in op.SCENES for s in op.sigmas()]


def test_joint_decision_collects_more_power(points):
    """the mean ratio joint / ref of the collected (true) power is above 1 on every scene; per set the objective the optimiser
    was given -- the power of its coefficient matrix -- does not fall by more than the allowance.  (Per set the TRUE power may
    fall at sigma > 0: the optimiser sees the noisy estimate.)  The sketch's 1.28 / 1.38 are printed beside, not asserted."""
    for pt in points:
        rec = op.record(pt)
        print("\n%s sigma %.1f: %.4f (sketch %.2f), objective %.4f" % (rec["scene"], rec["sigma"], rec["power_ratio_of_means"],
                                                                     rec["predicted_by_the_float64_sketch"],
                                                                     rec["objective_ratio_of_means"]))
        assert rec["power_ratio_of_means"] > 1.0
        G = pt["est"].shape[2] - 1
        allow = orf.decision_allowance(pt["est"], op.SWEEPS, True) * G * op.SWEEPS
        assert (pt["o_joint"] >= pt["o_ref"] - allow).all()
        assert (pt["o_joint"] / pt["o_ref"] >= 1.0 - allow / pt["o_ref"]).all()
        if pt["sigma"] == 0.0:                                     # the genie bound: the estimate is the truth up to rounding
            assert (pt["p_joint"] / pt["p_ref"]).min() > 0.999


def test_scene_traces_do_not_fall(points):
    for pt in points:
        G = pt["est"].shape[2] - 1
        allow, pb = orf.decision_allowance(pt["est"], op.SWEEPS, True), orf.power_bound(pt["est"], op.SWEEPS, True)
        drop = -np.diff(pt["res"]["power"].astype(np.float64), axis=1)
        assert (drop <= (G * allow + 2 * pb)[:, None]).all()
        assert (np.abs(pt["res"]["power"][:, -1] - pt["o_joint"]) <= pb).all()


# ---- the mutants ----

def one(q, bits, start=orf.START_ZERO, blocked=False, ci=None, mutant=None, sweeps=2):
    return orf.optimize_set(np.asarray(q, np.complex64), bits, sweeps, start, blocked, ci, mutant)


def check_own_term_removed(mutant=None):
    """d = 1, e = -1.2, start 0: r = 1, z = -1.2, so the code turns to 1; with the own term left in z = conj(s) e = +0.24"""
    codes, power, _ = one([[1, -1.2]], 1, mutant=mutant)
    assert codes.tolist() == [1] and abs(power[-1] - 4.84) < 1e-5


def check_conjugate(mutant=None):
    """d = j, e = 1: z = conj(j) = -j, the best phase is +j (code 1 of 4); without the conjugate it is -j and the power 0"""
    codes, power, _ = one([[1j, 1]], 2, mutant=mutant)
    assert codes.tolist() == [1] and power[-1] == 4


def check_state_updated(mutant=None):
    """d = 1, e = (-3, 1): group 0 turns, and group 1 must see the turned state (r = 4: it stays); on the old state it turns too"""
    codes, power, _ = one([[1, -3, 1]], 1, mutant=mutant)
    assert codes.tolist() == [1, 0] and power[-1] == 25


def check_tie_takes_lowest(mutant=None):
    """d = 1 - j, e = 1: z = 1 + j, codes 0 (phase 1) and 3 (phase -j) tie at 1; and z = 0 takes code 0 from a given 1"""
    assert one([[1 - 1j, 1]], 2, mutant=mutant)[0].tolist() == [0]
    assert one([[0, 1]], 1, orf.START_GIVEN, ci=np.array([1], np.uint8), mutant=mutant)[0].tolist() == [0]


def check_blocked_column_not_read(mutant=None):
    codes, power, _ = one([[5, -1]], 1, orf.START_REF, blocked=True, mutant=mutant)
    assert power.tolist() == [1, 1, 1]
    nan = one([[np.nan, -1]], 1, orf.START_REF, blocked=True, mutant=mutant)
    assert nan[1].tolist() == [1, 1, 1]


def check_rows_above_64(mutant=None):
    q = np.zeros((65, 2), np.complex64)
    q[64] = (1, -2)
    codes, power, _ = one(q, 1, mutant=mutant)
    assert codes.tolist() == [1] and power.tolist() == [1, 9, 9]


CHECKS = {"own": check_own_term_removed, "conj": check_conjugate, "state": check_state_updated, "tie": check_tie_takes_lowest,
          "blocked": check_blocked_column_not_read, "rows": check_rows_above_64}


@pytest.mark.parametrize("name", orf.MUTANTS)
def test_check_passes_on_the_restatement(name):
    CHECKS[name]()


@pytest.mark.parametrize("name", orf.MUTANTS)
def test_mutant_fails_the_check_named_for_it(name):
    with pytest.raises(AssertionError):
        CHECKS[name](name)


def test_mutation_table():
    """every check on the restatement and on every mutant: the check named for a mutant fails on it (the table that
    `pytest tests/test_irs_optimize_ref.py -k mutation_table -s` prints is kept as profiles/irs_optimize_mutations.txt)"""
    lines = ["mutant      " + "".join("%-32s" % f.__name__ for f in CHECKS.values())]
    for m in (None,) + orf.MUTANTS:
        row = []
        for name, f in CHECKS.items():
            try:
                f(m)
                row.append("pass")
            except AssertionError:
                row.append("FAIL")
            if m is None or name == m:
                assert row[-1] == ("pass" if m is None else "FAIL"), (m, name)
        lines.append("%-12s" % (m or "(none)") + "".join("%-32s" % r for r in row))
    print("\n" + "\n".join(lines))


# ---- the edges ----

def test_special_inputs():
    zero = orf.optimize(np.zeros((1, 3, 5), np.complex64), 2, 2)
    assert zero["codes"].tobytes() == bytes(4) and zero["power"].tobytes() == bytes(12) and zero["sweeps"][0] == 0
    q = crandn(np.random.default_rng(3), 1, 4, 6)
    q[0, 2, 3] = np.nan
    got = orf.optimize(q, 2, 2)                                    # a NaN row: every z is NaN, a NaN never replaces the maximum
    assert np.isnan(got["power"]).all() and (got["codes"] < 4).all()
    grp = irs.groups(4, 2)
    q = crandn(np.random.default_rng(4), 2, 3, 5)
    got = orf.optimize(q, 3, 1, group=grp)
    assert got["psi"].shape == (2, 16) and (got["psi"] == irs.PHASES[got["codes"][:, grp].astype(np.intp)]).all()
    given = orf.optimize(q, 1, 0, orf.START_GIVEN, codes_in=np.full((2, 4), 0xFF, np.uint8))
    assert (given["codes"] == 1).all()                             # only the low B bits of a given code count
