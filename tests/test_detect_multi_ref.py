"""NUMERICS.md rule 24 (joint detection over A sample-synchronous antennas) on the CPU: the restatement of
tests/detect_multi_ref.py against rule 3's (tests/detect_ref.py), against the float64 definition, on the exact-threshold
construction of tests/detect_rows.py, on the Rayleigh scene the rule quotes, and three mutants of the restatement, each of
which must fail the test named for it (profiles/stream_diversity_mutations.txt)."""
import math
import os

import numpy as np
import pytest

import detect_multi_ref as mr
import detect_ref as dr
import detect_rows as rows
import stream_diversity_rows as sdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, MP = 0.56, 2


def _bits_equal(a, b):
    return all(np.array_equal(np.asarray(u).view(np.uint32), np.asarray(v).view(np.uint32)) for u, v in zip(a, b))


def _floats(n=3000, seed=5):
    """a stream whose summation order matters: frames in noise, levels a decade apart"""
    x = sdr.capture(1)[0][:n].astype(np.complex64)
    rng = np.random.default_rng(seed)
    return (x * rng.uniform(0.3, 3.0, n)).astype(np.complex64)


def test_one_antenna_is_rule_3_bit_for_bit():
    for x in (sdr.capture(1)[0], _floats(), rows.stream_rows(2, "unit")[0]["x"][:6000]):
        assert _bits_equal(mr.window_sums([x]), dr.window_sums(x))
        for thr in (THR, rows.NEXT75, 0.75, 0.0):
            assert np.array_equal(mr.bits([x], thr), dr.above(*dr.window_sums(x), thr)[0])
        t, Ar, Ai = mr.detect([x], THR, MP)
        t1, Ar1, Ai1 = dr.detect(x, THR, MP)
        assert np.array_equal(t, t1) and _bits_equal((Ar, Ai), (Ar1, Ai1))


def _copies_hold(n_ant, mutant=None):
    """A identical antennas: the joint sums are exactly A times the single-antenna sums, the triggers the same"""
    x = _floats()
    one = dr.window_sums(x)
    got = mr.window_sums([x] * n_ant, mutant)
    exact = all(np.array_equal(g, np.float32(n_ant) * o) for g, o in zip(got, one))
    return exact and np.array_equal(mr.detect([x] * n_ant, THR, MP, mutant)[0], dr.detect(x, THR, MP)[0])


@pytest.mark.parametrize("n_ant", [2, 4, 8])
def test_identical_copies_give_exact_multiples_and_the_same_triggers(n_ant):
    assert _copies_hold(n_ant)
    # and with them the coarse CFO: atan2 of (A Ai, A Ar) is that of (Ai, Ar) up to its own rounding of the quotient, which a
    # power of two leaves alone
    x = _floats()
    t, Ar, Ai = mr.detect([x] * n_ant, THR, MP)
    _, Ar1, Ai1 = dr.detect(x, THR, MP)
    assert len(t) > 0 and np.array_equal(Ar, np.float32(n_ant) * Ar1) and np.array_equal(Ai, np.float32(n_ant) * Ai1)


@pytest.mark.parametrize("n_ant", [2, 3, 5, 6, 8])
def test_an_all_zero_antenna_changes_no_bit(n_ant):
    """s + 0 = s exactly.  A zero antenna behind the others leaves the tree's other additions as they are (an odd one out moves
    up unchanged), so the sums, the bits and the triggers are those of the antennas without it; with two antennas that
    holds for either place.  Anywhere else the summands' sums are those of the same tree with that leaf adding nothing."""
    xs = list(sdr.capture(n_ant - 1))
    z = np.zeros_like(xs[0])
    assert _bits_equal(mr.window_sums(xs + [z]), mr.window_sums(xs))
    assert np.array_equal(mr.bits(xs + [z], THR), mr.bits(xs, THR))
    assert np.array_equal(mr.detect(xs + [z], THR, MP)[0], mr.detect(xs, THR, MP)[0])
    if n_ant == 2:
        assert _bits_equal(mr.window_sums([z] + xs), dr.window_sums(xs[0]))
        assert np.array_equal(mr.detect([z] + xs, THR, MP)[0], dr.detect(xs[0], THR, MP)[0])
    for where in range(n_ant):
        parts = [mr.summands(x) for x in xs[:where] + [z] + xs[where:]]
        for c in range(3):
            # (equal as values: a summand that is -0 becomes +0 beside the zero antenna, which no window sum can show --
            # it would need -0 in every term of three consecutive blocks, tests/detect_rows.py)
            assert np.array_equal(mr.tree_sum([p[c] for p in parts]), _tree_without(parts, c, where))


def _tree_without(parts, c, where):
    """the tree over all places with place `where` contributing no addition: its sibling moves up as it is"""
    v = [None if k == where else np.asarray(p[c], np.float32) for k, p in enumerate(parts)]
    while len(v) > 1:
        nxt = []
        for i in range(len(v) // 2):
            a, b = v[2 * i], v[2 * i + 1]
            nxt.append(b if a is None else a if b is None else a + b)
        if len(v) & 1:
            nxt.append(v[-1])
        v = nxt
    return v[0]


def rounding_count(n_ant):
    """Roundings on the deepest path from a product to a window sum, per component.
    Summand: the product (re re', rounded) and the fma that adds the second product (one rounding): 2.
    Tree: ceil(log2 A) additions above a leaf.
    Window: a term inside H or S passes the four levels of the Kogge-Stone scan (steps 1, 2, 4, 8), then the three additions
    ((T + B) + B) + H of the 48-sample window: 7.  (The 64-sample window has a fourth block total, hence eight additions on
    its deepest path; the rule's count of 7 is asserted for P as well, which only asks more.)
    Each rounding is at most 2^-24 relative to a partial sum whose magnitude the window's sum of absolute terms bounds."""
    return 2 + math.ceil(math.log2(n_ant)) + 7


@pytest.mark.parametrize("n_ant", [1, 2, 3, 4, 8])
def test_within_the_rounding_count_of_the_float64_definition(n_ant):
    xs = sdr.capture(n_ant)
    got, want, scale = mr.window_sums(xs), mr.definition(xs), mr.abs_terms(xs)
    bound = rounding_count(n_ant) * 2.0 ** -24
    for g, w, s in zip(got, want, scale):
        err = np.abs(g.astype(np.float64) - w)
        assert (err <= bound * s).all(), float((err / np.maximum(s, 1e-300)).max() / 2.0 ** -24)


@pytest.mark.parametrize("n_ant", [1, 2, 3, 8])
def test_a_sample_exactly_on_the_threshold_stays_strict(n_ant):
    """unit bursts (tests/detect_rows.py) on every antenna, each rotated by its own power of j: every joint sum is a small
    integer, |A| / P is exactly 48 / 64 on the plateau.  0.75 is never exceeded, nextafter(0.75f, 0) is."""
    x = rows.stream_rows(2, "unit")[0]["x"][:12000]
    xs = [(x * (1j ** a)).astype(np.complex64) for a in range(n_ant)]
    one = dr.above(*dr.window_sums(x), rows.NEXT75)[0]
    assert one.any()
    assert not mr.bits(xs, 0.75).any()
    assert np.array_equal(mr.bits(xs, rows.NEXT75), one)
    assert np.array_equal(mr.detect(xs, rows.NEXT75, 2)[0], dr.detect(x, rows.NEXT75, 2)[0])
    assert len(mr.detect(xs, 0.75, 2)[0]) == 0


@pytest.fixture(scope="module")
def scene_counts():
    xs, starts = sdr.rayleigh_scene()
    single = [sdr.frames_detected(dr.detect(x, THR, MP)[0], starts) for x in xs]
    joint = {a: sdr.frames_detected(mr.detect(xs[:a], THR, MP)[0], starts) for a in (2, 4)}
    return single, joint, xs, starts


def test_rayleigh_scene_joint_detection_finds_more_frames_at_10_db(scene_counts):
    single, joint, _, starts = scene_counts
    print("frames detected of %d: single %s, joint 2: %d, joint 4: %d" % (len(starts), single, joint[2], joint[4]))
    assert joint[4] >= joint[2] >= max(single)
    assert max(single) < len(starts)            # the scene is not saturated: there is something to gain


# ---- the mutants: each must fail the property named for it ----

def test_mutant_left_to_right_sum_fails_the_exact_copies():
    m = "left-to-right sum"
    assert _copies_hold(8) and not _copies_hold(8, m)
    xs = sdr.capture(8)
    assert not _bits_equal(mr.window_sums(xs, m), mr.window_sums(xs))          # what the device is compared on
    _recorded(m)


def test_mutant_windows_before_the_antenna_sum_fails_the_bit_pattern():
    m = "windows before the antenna sum"
    for a in (2, 3, 8):
        xs = sdr.capture(a)
        assert not _bits_equal(mr.window_sums(xs, m), mr.window_sums(xs)), a    # what the device is compared on
    _recorded(m)


def test_mutant_threshold_per_antenna_or_ed_fails_the_joint_triggers(scene_counts):
    m = "threshold per antenna OR-ed"
    xs = sdr.capture(2)
    assert not np.array_equal(mr.bits(xs, THR, m), mr.bits(xs, THR))           # what the device is compared on
    # one strong antenna beside one of noise alone: the OR keeps the strong antenna's plateau, the joint metric is diluted
    x = rows.stream_rows(2, "unit")[0]["x"][:12000]
    noise = sdr.antenna(np.zeros(x.size), noise_seed=9) * np.float32(3)
    assert len(mr.detect([x, noise], rows.NEXT75, 2, m)[0]) > len(mr.detect([x, noise], rows.NEXT75, 2)[0])
    _recorded(m)


def _recorded(mutant):
    txt = open(os.path.join(ROOT, "profiles", "stream_diversity_mutations.txt")).read()
    assert mutant in txt


def test_reference_imports_nothing_of_the_product_or_the_oracle():
    src = open(os.path.join(ROOT, "tests", "detect_multi_ref.py")).read()
    for word in ("wifirx", "oracle", "capi", "ctypes"):
        assert ("import " + word) not in src and ("from " + word) not in src
