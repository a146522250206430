"""The oracle's SPEC mode against the float64 restatement of the prose: LMS / COMB / STA, points, LLRs, CSI, moments, bw/fc.

Every GPU test of the receive chain asserts "HIP == oracle, bit for bit", and oracle and kernels were written by one hand
from one set of tables.  `tests/independent_rx.py` shares nothing with either; `tests/test_independent_rx.py` holds its hard
decisions of the LS equaliser against the oracle at the default operating point.  This module holds the rest: the three
other equalisers as NUMERICS.md rule 11 states them in words, the equalised points, the LLRs of rule 7, the channel-state
weight of rule 12, the CSI export and the moments of rule 13 -- at three (bandwidth, frequency) operating points, because
bandwidth / frequency scales the sampling-offset compensation of every symbol (rule 9) and no other test leaves the default.
Cases, tolerances and the rule for which symbols are compared: `tests/independent_eq_cases.py`.

The mutants are text substitutions in the reference's source: a wrong constant, edge rule or update order that oracle and
kernel might share must move the compared quantity by at least 10 x its tolerance on at least one case, or this module
could not see it.  `profiles/independent_eq_distances.json` and `profiles/independent_eq_mutations.txt` are what a run with
WIFIRX_RECORD_DISTANCES=1 writes; the tolerances are held against the former below.

The device against the same reference, without the oracle in between: `tests/test_gpu_independent_eq.py`."""
import json
import math
import os
import types

import numpy as np
import pytest

import independent_eq_cases as C

RECORD = os.environ.get("WIFIRX_RECORD_DISTANCES") == "1"
_moved = {}


@pytest.mark.parametrize("op", C.OPS, ids=lambda op: "%gMHz_%gGHz" % (op[0] / 1e6, op[1] / 1e9))
@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_spec_mode_agrees_with_the_reference(orc, name, op):
    for ce in range(4):
        out = C.distances(C.reference(name, ce, op), C.oracle_outputs(orc, name, ce, op), ce)
        print(name, op, C.EQ_NAMES[ce], out)
        C.check(out, (name, op, C.EQ_NAMES[ce]))


def _measure_all(orc):
    """{equaliser: {operating point: {quantity: largest distance over the cases}}}, the smallest share of compared symbols"""
    table, share = {}, 1.0
    for ce in range(4):
        for op in C.OPS:
            row = dict.fromkeys(C.QUANTITIES, 0.0)
            for name in C.CASES:
                out = C.distances(C.reference(name, ce, op), C.oracle_outputs(orc, name, ce, op), ce)
                share = min(share, out["share"])
                for q in C.QUANTITIES:
                    row[q] = max(row[q], out[q] or 0.0)
            table.setdefault(C.EQ_NAMES[ce], {})["bw=%g fc=%g" % op] = row
    largest = {q: max(r[q] for e in table.values() for r in e.values()) for q in C.QUANTITIES}
    return dict(delta=C.DELTA, smallest_share_of_compared_symbols=share, largest=largest, by_equaliser=table)


def _write(name, text):
    """a recording run (WIFIRX_RECORD_DISTANCES=1) rewrites the file under profiles/; an ordinary run writes nothing"""
    if RECORD:
        with open(os.path.join(C.ROOT, "profiles", name), "w") as f:
            f.write(text)


def test_tolerances_are_four_times_the_recorded_distances(orc):
    now = _measure_all(orc)
    _write("independent_eq_distances.json", json.dumps(now, indent=1) + "\n")
    with open(C.DISTANCES) as f:
        rec = json.load(f)
    for q in C.QUANTITIES:
        if q != "llr":                                                        # the unweighted LLRs are held to the points' tolerance
            assert math.isclose(C.TOL[q], 4 * rec["largest"][q], rel_tol=1e-3), q
        else:
            assert 4 * rec["largest"][q] <= C.TOL[q], q
        assert now["largest"][q] <= C.TOL[q], (q, now["largest"])
    assert math.isclose(C.DELTA, 16 * rec["largest"]["points"], rel_tol=1e-3)
    assert math.isclose(rec["delta"], C.DELTA, rel_tol=1e-12)                 # the record was made with this margin


# name: (text, replacement, equalisers, the quantity whose assertion is meant to fail)
MUTANTS = {
    "lms_step_0.4": ("LMS_STEP = 0.5 ", "LMS_STEP = 0.4 ", (1,), "points"),
    "comb_alpha_0.25": ("COMB_ALPHA = 0.2 ", "COMB_ALPHA = 0.25 ", (2,), "points"),
    "comb_edges_from_the_nearest_pilot": ("lo_edge = hi_edge = nodes.mean(axis=1)", "lo_edge, hi_edge = nodes[:, 0], nodes[:, 3]",
                                          (2,), "points"),
    "comb_first_symbol_smoothed_like_the_others": ("Hc if s == 0 else", "Hc if s < 0 else", (2,), "points"),
    "sta_divides_by_5_everywhere": ("avg = tot / np.maximum(cnt, 1.0)[None, :]", "avg = tot / 5.0", (3,), "points"),
    "sta_updates_before_equalising": ("H_used = DH ", "H_used = DH_new ", (3,), "points"),
    "rule9_iir_0.8_0.2": ("0.9 * d_er + 0.1 * er_new", "0.8 * d_er + 0.2 * er_new", (0, 1, 2, 3), "points"),
    "frequency_off_by_5.89/2.412": ("float(bandwidth), float(frequency),", "float(bandwidth), float(frequency) * 5.89 / 2.412,",
                                    (0, 1, 2, 3), "points"),
    "qam64_L2_4a_and_2a_swapped": ("2 * a - np.abs(np.abs(u) - 4 * a)", "4 * a - np.abs(np.abs(u) - 2 * a)", (0,), "llr"),
    "csi_weight_from_the_running_H": ("wH = H_ls ", "wH = H_run ", (1, 2, 3), "llr_csi_rel"),
}


def mutated(text, replacement):
    path = os.path.join(C.ROOT, "tests", "independent_rx.py")
    src = open(path).read()
    assert src.count(text) == 1, text
    mod = types.ModuleType("independent_rx_mutant")
    mod.__file__ = path
    exec(compile(src.replace(text, replacement), path, "exec"), mod.__dict__)
    return mod.IndependentRx


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_of_the_reference_is_caught(orc, mutant):
    text, replacement, equalisers, quantity = MUTANTS[mutant]
    rx_class = mutated(text, replacement)
    op = C.DEFAULT_OP
    moved = {}
    for ce in equalisers:
        for name in C.CASES:
            try:
                out = C.distances(C.reference(name, ce, op, rx_class=rx_class, cache=False), C.oracle_outputs(orc, name, ce, op), ce)
                moved[(C.EQ_NAMES[ce], name)] = out[quantity]
            except AssertionError as e:                      # a mutant may also break the records
                moved[(C.EQ_NAMES[ce], name)] = "records: %s" % e
    _moved[mutant] = moved
    _record_mutants()
    print(mutant, moved)
    figures = [v for v in moved.values() if isinstance(v, float)]
    assert max(figures) >= 10 * C.TOL[quantity], (mutant, moved)


def _record_mutants():
    """the figures of the mutants run so far, as text (profiles/independent_eq_mutations.txt is the full list's)"""
    lines = ["Mutants of tests/independent_rx.py (text substitutions, tests/test_independent_eq.py) against the oracle's SPEC mode at",
             "bw=%g fc=%g: the largest distance of the quantity whose assertion is meant to fail, per equaliser and case." % C.DEFAULT_OP,
             "Unmutated, the largest distances are those of independent_eq_distances.json; a mutant is caught at >= 10 x the tolerance.", ""]
    for m, moved in _moved.items():
        text, replacement, _, quantity = MUTANTS[m]
        lines.append("%s   [%s -> %s]   quantity: %s, tolerance %.3g" % (m, text.strip(), replacement.strip(), quantity, C.TOL[quantity]))
        for (eq, name), v in moved.items():
            lines.append("    %-5s %-10s %s" % (eq, name, ("%.3g" % v) if isinstance(v, float) else v))
    _write("independent_eq_mutations.txt", "\n".join(lines) + "\n")
