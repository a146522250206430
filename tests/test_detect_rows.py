"""The detect phase on host-built inputs, CPU part: the restatement of tests/detect_ref.py (NUMERICS.md rule 3 + SURVEY.md
App. A.2) against the oracle on every entry of tests/detect_rows.py; the float64 definition on the exact classes; the
honesty conditions of the table, asserted on the reference alone; mutants of the reference, each of which must break the
equality on a named entry (profiles/detect_rows_mutations.txt)."""
import ast
import os
from fractions import Fraction

import numpy as np
import pytest

import detect_ref as ref
import detect_rows as rows

F16 = np.float32(16)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rn32(v):
    """a Fraction rounded to the nearest float32, ties to even (exact integer arithmetic)"""
    if v == 0:
        return np.float32(0)
    sgn, v = (-1 if v < 0 else 1), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    e -= Fraction(2) ** e > v
    e = max(e, -126)
    q = v / Fraction(2) ** (e - 23)
    n, r = divmod(q.numerator, q.denominator)
    r = Fraction(r, q.denominator)
    n += r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1)
    return np.float32(sgn * float(Fraction(n) * Fraction(2) ** (e - 23)))


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(3000) * 10.0 ** rng.integers(-20, 20, 3000)).astype(np.float32)
    b = (rng.standard_normal(3000) * 10.0 ** rng.integers(-18, 18, 3000)).astype(np.float32)
    c = (rng.standard_normal(3000) * 10.0 ** rng.integers(-30, 30, 3000)).astype(np.float32)
    c[:1000] = (-(a[:1000].astype(np.float64) * b[:1000])).astype(np.float32)          # cancellation: the low product bits decide
    # ties: a b = an odd multiple of half an ulp of c's binade, plus or minus one unit 2^-46 that only a fused operation
    # sees.  a = 1 + k 2^-23, b = 1 + 2^-23 => a b = 1 + (k + 1) 2^-23 + k 2^-46; c = 2^24 puts the tie at 1 (ulp 2)
    k = rng.integers(1, 1 << 22, 500)
    ta = (1 + k * 2.0 ** -23).astype(np.float32)
    tb = np.full(500, 1 + 2.0 ** -23, np.float32)
    tc = np.where(k & 1, 2.0 ** 24, -2.0 ** 24).astype(np.float32)
    a, b, c = np.concatenate([a, ta, -ta]), np.concatenate([b, tb, tb]), np.concatenate([c, tc, tc])
    got = ref.fma32(a, b, c)
    want = np.array([rn32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(u32(got), u32(want))
    two = np.float32(a * b) + c                                             # the unfused form differs somewhere: the test can see
    assert not np.array_equal(u32(two), u32(want))


def test_reference_imports_nothing_of_the_product_or_the_oracle():
    src = open(os.path.join(os.path.dirname(__file__), "detect_ref.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods == {"numpy"}


def streams_of(mp, cls):
    """(name, samples, thr, first_only) of every table entry -- every slot of a batch row, every stream row -- with
    first_only on and off"""
    for r in rows.batch_rows(mp, cls):
        for k, s in enumerate(rows.slots_of(r)):
            yield "%s[%d]" % (r["name"], k), s, r["thr"], True
            yield "%s[%d]" % (r["name"], k), s, r["thr"], False
    for r in rows.stream_rows(mp, cls):
        yield r["name"], r["x"], r["thr"], True
        yield r["name"], r["x"], r["thr"], False


_sums = {}


def sums(name, x):
    if name not in _sums:
        _sums[name] = ref.window_sums(x)
    return _sums[name]


@pytest.mark.parametrize("cls", rows.CLASSES)
@pytest.mark.parametrize("mp", rows.PLATEAUS)
def test_restatement_equals_oracle(orc, mp, cls):
    n_trig = 0
    for name, x, thr, first in streams_of(mp, cls):
        Ar, Ai, P = sums(name, x)
        t = np.asarray(ref.sync_short(ref.above(Ar, Ai, P, thr)[0], mp, first), dtype=np.int64)
        ot, oc = orc.sync_short(x, thr, mp, orc.MATH_SPEC, first_only=first, cap=8192)
        assert np.array_equal(t, ot), name
        assert np.array_equal(u32(orc.atan2(Ai[t], Ar[t]) / F16), u32(oc)), name
        n_trig += len(t)
    assert n_trig > 20


@pytest.mark.parametrize("cls", rows.EXACT)
@pytest.mark.parametrize("mp", rows.PLATEAUS)
def test_exact_classes_equal_the_float64_definition_and_libm(orc, mp, cls):
    for name, x, thr, first in streams_of(mp, cls):
        Ar, Ai, P = sums(name, x)
        bits = ref.above(Ar, Ai, P, thr)[0]
        dr, di, dp = ref.definition(x)
        assert np.array_equal(dr, Ar) and np.array_equal(di, Ai) and np.array_equal(dp, P), name
        tp = float(np.float32(thr)) * dp
        with np.errstate(over="ignore"):
            dbits = dr * dr + di * di > tp * tp
        assert np.array_equal(dbits, bits), name
        t = ref.sync_short(bits, mp, first)
        assert ref.sync_short(dbits, mp, first) == t
        lt, _ = orc.sync_short(x, thr, mp, orc.MATH_LIBM, first_only=first, cap=8192)
        assert np.array_equal(lt, np.asarray(t, dtype=np.int64)), name


def runs_of(bits):
    """(start, length) of the maximal runs of set bits"""
    b = np.concatenate([[0], np.asarray(bits, dtype=np.int8), [0]])
    d = np.diff(b)
    s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return list(zip(s.tolist(), (e - s).tolist()))


@pytest.mark.parametrize("mp", rows.PLATEAUS)
def test_honesty_conditions(orc, mp):
    """what the table must contain for this min_plateau, found in the restated reference's own bits and triggers"""
    seen = dict(run_short=0, run_hit=0, t16_0=0, t16_15=0, tile=0, span=0, sup480=0, acc481=0, eq=0, eq50=0, eq75=0, b_tile=0)
    angles = []
    for cls in rows.CLASSES:
        for name, x, thr, first in streams_of(mp, cls):
            is_stream = not name.endswith("]")
            Ar, Ai, P = sums(name, x)
            bits, m2, tp2 = ref.above(Ar, Ai, P, thr)
            trig = ref.sync_short(bits, mp, first)
            eq = (m2 == tp2) & (m2 > 0)
            seen["eq"] += int(eq.sum())
            seen["eq50"] += int(eq.sum()) if thr == 0.5 else 0
            seen["eq75"] += int(eq.sum()) if thr == 0.75 else 0
            if first:
                continue
            tset = set(trig)
            for s, L in runs_of(bits):
                inside = [t for t in trig if s <= t < s + L]
                seen["run_short"] += L == mp and not inside
                seen["run_hit"] += L == mp + 1 and inside == [s + L - 1]
            for t in trig:
                seen["t16_0"] += t % 16 == 0
                seen["t16_15"] += t % 16 == 15
                seen["b_tile"] += (not is_stream) and t % 64 < mp
                seen["tile"] += is_stream and t % 64 < mp
                seen["span"] += is_stream and t % 1024 < mp
                if cls == "unit":
                    angles.append(float(np.arctan2(np.float64(Ai[t]), np.float64(Ar[t]))))
            if is_stream and len(trig):
                # a hit: mp + 1 set bits end here.  One exactly 480 behind a trigger must be ignored, one 481 behind taken
                c = np.concatenate([[0], np.cumsum(bits)])
                for t in trig:
                    for d in (480, 481):
                        p = t + d
                        if p < bits.size and p - mp >= 0 and c[p + 1] - c[p - mp] == mp + 1 and not bits[p - mp - 1]:
                            if d == 480:
                                assert p not in tset, name
                                seen["sup480"] += 1
                            else:
                                seen["acc481"] += p in tset
    need = ["run_hit", "t16_0", "t16_15", "sup480", "acc481", "eq", "eq50", "eq75"]
    if mp > 0:          # a run of 0 samples and a residue below 0 do not exist
        need += ["run_short", "tile", "span", "b_tile"]
    assert all(seen[k] > 0 for k in need), (mp, seen)
    a = np.array(angles)
    for want in (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi):           # rot 0, 1, 3, and 2 with both signs of pi
        assert (np.abs(a - want) < 1e-6).any(), (mp, want)
    assert (np.abs(np.abs(a) - np.pi) < 1e-6).sum() >= 4
    # a burst on its own: the angle its rot announces
    r = [r for r in rows.batch_rows(mp, "unit") if r["name"].startswith("edges/")][0]
    n = 0
    for rot, x in zip(r["rots"], rows.slots_of(r)):
        t, Ar, Ai = ref.detect(x, r["thr"], mp, first_only=True)
        for k in range(len(t)):
            ang = float(np.arctan2(np.float64(Ai[k]), np.float64(Ar[k])))
            assert abs((abs(ang) if rot == 2 else ang) - (0.0, np.pi / 2, np.pi, -np.pi / 2)[rot]) < 1e-6, (mp, rot, ang)
            n += 1
    assert n >= 20


def test_thresholds_and_plateaus_are_the_issue_lists():
    assert rows.PLATEAUS == (0, 1, 2, 3, 15, 16, 17, 31, 32)
    assert [np.float32(t) for t in rows.THRS] == [np.float32(t) for t in (0, 1e-30, 0.35, 0.5, 0.56, np.nextafter(np.float32(0.75), np.float32(0)), 0.75, 1.0, 1.5, 1e19)]
    for mp in rows.PLATEAUS:
        for cls in rows.CLASSES:
            for form in (rows.batch_rows, rows.stream_rows):
                assert {np.float32(r["thr"]) for r in form(mp, cls)} >= {np.float32(t) for t in rows.THRS}
            assert all(r["x"].size <= 60000 for r in rows.stream_rows(mp, cls))
            assert all(len(s) <= 2048 for r in rows.batch_rows(mp, cls) for s in rows.slots_of(r))
    # the wave whose four slots trigger in block 4, in block 120, never, and have length 0
    for mp in rows.PLATEAUS:
        for name in ("wave4/", "wave4u/"):
            r = [r for r in rows.batch_rows(mp, "unit") if r["name"].startswith(name)][0]
            t = [ref.detect(s, r["thr"], mp, first_only=True)[0] for s in rows.slots_of(r)]
            assert [int(v[0]) // 16 if len(v) else None for v in t] == [4, 120, None, None]
            assert [len(s) for s in rows.slots_of(r)] == [2048, 2048, 2048, 0 if name == "wave4/" else 2048]
    # 1e-30 underflows (thr P)^2 to 0 and 1e19 overflows it to inf wherever A != 0, on every class
    for cls in rows.CLASSES:
        r = [r for r in rows.stream_rows(2, cls) if r["name"].startswith("thr/")][0]
        Ar, Ai, P = ref.window_sums(r["x"])
        nz = (Ar != 0) | (Ai != 0)
        assert nz.any() and (P[nz] >= 2).all()
        assert (ref.above(Ar, Ai, P, 1e-30)[2] == 0).all() and np.isinf(ref.above(Ar, Ai, P, 1e19)[2][nz]).all()


# mutant of the reference -> the entry (min_plateau, class, name) on which it must part from the oracle
MUTANTS = {
    ">= for >": (2, "unit", "thr/unit/mp2/thr0.75"),
    "plateau <= min_plateau": (2, "unit", "main/unit/mp2"),
    "copied >= MIN_GAP": (2, "unit", "main/unit/mp2"),
    "windows of 47 / 63 samples": (2, "unit", "main/unit/mp2"),
    "suffix T[r] = S[r]": (2, "unit", "main/unit/mp2"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_reference_mutants_part_from_the_oracle(orc, mutant):
    mp, cls, name = MUTANTS[mutant]
    r = [r for r in rows.stream_rows(mp, cls) if r["name"] == name][0]
    x, thr = r["x"], r["thr"]
    tail = {"windows of 47 / 63 samples": 2, "suffix T[r] = S[r]": 0}.get(mutant, 1)
    Ar, Ai, P = ref.window_sums(x, tail=tail)
    bits = ref.above(Ar, Ai, P, thr, ge=mutant == ">= for >")[0]
    t = ref.sync_short(bits, mp, plateau_le=mutant == "plateau <= min_plateau", gap_ge=mutant == "copied >= MIN_GAP")
    ot, _ = orc.sync_short(x, thr, mp, orc.MATH_SPEC, cap=8192)
    assert not np.array_equal(np.asarray(t, dtype=np.int64), ot), mutant
    txt = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "profiles", "detect_rows_mutations.txt")).read()
    assert mutant in txt and name in txt
