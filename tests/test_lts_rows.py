"""Frame synchronisation on host-built slots, CPU part: the restatement of tests/lts_ref.py (NUMERICS.md rules 2, 6, 8 and
SURVEY.md App. A.3) against the oracle on every row of tests/lts_rows.py -- the record, the four peaks of the oracle's
dbg_top4 / dbg_mag4 hook --, against the search's float64 definition where the row allows it, the table's conditions
asserted on the restatement alone, and the mutants of the reference, each of which must change the record of a named row
(profiles/lts_rows_mutations.txt)."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

import detect_ref
import lts_ref as ref
import lts_rows as rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = np.float32(np.pi)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restated(orc, row, mut=(), total=None):
    return rows.restate(row, orc.sincos, orc.atan2, mut, total)


def record(f):
    """what a mutant must change: flags, frame_start, the bits of cfo_fine"""
    return int(f["flags"]), int(f["frame_start"]), int(u32(f["cfo_fine"]).reshape(-1)[0])


_oracle = {}


def oracle_row(orc, row, lts_search=0):
    """(frame record, top four lags, their magnitudes) of the oracle's SPEC mode on the row as a slot"""
    key = (row["name"], lts_search)
    if key not in _oracle:
        x = rows.slot_of(row)
        top, mag = np.full(4, -9, np.int32), np.zeros(4, np.float32)
        prm = orc.make_params(threshold=row["thr"], min_plateau=row["mp"], max_sym=1, lts_search=lts_search)
        prm.dbg_top4 = top.ctypes.data_as(C.c_void_p).value
        prm.dbg_mag4 = mag.ctypes.data_as(C.c_void_p).value
        fr = orc.demod_batch(x, x.size, prm)["frames"][0]
        _oracle[key] = (fr, top, mag)
    return _oracle[key]


def _table(name, conv):
    txt = open(os.path.join(ROOT, "include", "wifirx_tables.h")).read()
    m = re.search(r"%s\[\d+\] = \{(.*?)\};" % name, txt, re.S)
    return [conv(v.strip()) for v in m.group(1).replace("\n", " ").split(",") if v.strip()]


def test_taps_are_the_tables_bit_for_bit():
    lt, lq = ref.taps()
    t = np.array(_table("WR_LTS_TIME", lambda v: float.fromhex(v.rstrip("f"))), np.float32).reshape(64, 2)
    q = np.array(_table("WR_LTS_Q8", int), np.int64).reshape(64, 2)
    assert np.array_equal(u32(lt), u32(t)) and np.array_equal(lq, q)
    # the two real taps the `cfo` figures stand on, with a +0 imaginary part
    assert lt[0, 0] == -lt[32, 0] and u32(lt[[0, 32], 1]).tolist() == [0, 0]


def test_atan2_takes_the_sign_of_a_zero(orc):
    """rule 1: (-0, x < 0) is -pi and (-0, x > 0) is -0, as atan2f and the float64 definition say (the rows cfo/fig64/-1/+
    and cfo/fig65/-1/+ bring the device there); a NaN of either sign stays a NaN"""
    y = np.array([-0.0, 0.0, -0.0, 0.0, -0.0, 0.0], np.float32)
    x = np.array([-1, -1, 1, 1, -np.inf, np.inf], np.float32)
    assert np.array_equal(u32(orc.atan2(y, x)), u32(np.arctan2(y.astype(np.float64), x.astype(np.float64))))
    nan = np.array([0x7fc00000, 0xffc00000], np.uint32).view(np.float32)
    assert np.isnan(orc.atan2(nan, np.ones(2, np.float32))).all()


def test_reference_imports_nothing_of_the_product_or_the_oracle():
    mods = set()
    for node in ast.walk(ast.parse(open(os.path.join(os.path.dirname(__file__), "lts_ref.py")).read())):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods == {"numpy", "detect_ref"}


def test_names_are_unique_and_slots_small():
    names = [r["name"] for r in rows.table()]
    assert len(names) == len(set(names)) and 100 < len(names) < 400
    assert all(rows.slot_of(r).size <= rows.SLOT for r in rows.table())
    assert rows.PUSHES == (7, 16, 63, 64, 65, 100, 777, 4096, 0) and rows.STREAM_BATCHES == (0, 20000)


@pytest.mark.parametrize("cls", ["ties", "shortcut", "pair", "cfo", "q8", "edges"])
def test_restatement_equals_oracle(orc, cls):
    n = 0
    for r in [r for r in rows.table() if r["cls"] == cls]:
        f = restated(orc, r)
        fr, top, mag = oracle_row(orc, r)
        name = r["name"]
        assert len(f["triggers"]) == 1, name                    # one trigger per row: it can stand in a stream
        assert fr["trigger"] == f["t"] and u32(fr["cfo_coarse"]) == u32(f["cfo_c"]), name
        keep = ref.F_DETECTED | ref.F_SYNC | (ref.F_TRUNCATED if f["L"] < 383 else 0)
        assert (int(fr["flags"]) & keep, int(fr["frame_start"]), int(u32(fr["cfo_fine"])[0])) == record(f), (name, fr, record(f))
        assert not any(np.isnan(fr[k]) for k in ("cfo_coarse", "cfo_fine", "snr_db")), name      # a NaN's bits are nobody's rule
        if f["L"] >= 383:
            assert top.tolist() == f["top"] and np.array_equal(u32(mag), u32(f["top_mag"])), (name, top, f["top"])
            if "burst" not in r and f["cfo_c"] == 0 and np.isfinite(f["xr"]).all() and np.isfinite(f["xi"]).all():
                assert np.array_equal(f["yr"], f["xr"]) and np.array_equal(f["yi"], f["xi"]), name   # cfo_c = 0: y == x
        n += 1
    assert n >= 8


def test_float64_definition_where_the_row_allows_it(orc):
    """same frame start; the CFO within rule 1's bound on sp_atan2 (4e-7), one division by diff and the result's rounding.
    Rows with f64 = False: exact ties (the float64 sums do not tie), non-finite samples, overflowed magnitudes, and the
    d = 63 figures and `near` copies whose ranking hangs on the last float32 bit."""
    n = 0
    for r in rows.table():
        f = restated(orc, r)
        if not r["f64"] or f["L"] < 383:
            continue
        found, fs, cfo = ref.definition(rows.slot_of(r), f["t"], f["cfo_c"])
        assert found == f["found"] and (fs if found else 0) == f["frame_start"], (r["name"], found, fs, f["found"], f["frame_start"])
        if found:
            got = float(f["cfo_fine"])
            assert abs(got - cfo) <= 4e-7 / found + 2.0 ** -24 * abs(got), (r["name"], got, cfo)
        # and the oracle's exhaustive float32 search agrees with rule 6 on the record
        assert oracle_row(orc, r, 1)[0] == oracle_row(orc, r, 0)[0], r["name"]
        n += 1
    assert n >= 50


lane_of = ref.lane_of


def test_table_conditions(orc):
    seen = dict(short=0, wide=0, wide_other_pair=0)
    founds, args = set(), set()
    for r in rows.table():
        f, w, name = restated(orc, r), r["want"], r["name"]
        if "L" in w:
            assert f["L"] == w["L"] and bool(f["flags"] & ref.F_TRUNCATED) == (w["L"] < 383), name
        if f["L"] < 383:
            continue
        tied = np.flatnonzero(f["mag1"] == f["mag1"].max())
        lanes = [lane_of(int(i)) for i in tied]
        if w.get("tie_lanes"):
            assert len(set(lanes)) >= 2, name
        if w.get("tie_lane"):
            assert len(lanes) > len(set(lanes)), name
        if w.get("rise"):
            assert len(tied) >= 9 and f["top"] == sorted(f["cand"])[:3:-1] and not f["shortcut"], (name, f["cand"], f["top"])
        elif r["cls"] == "ties":
            assert f["top"][1] >= 0 and u32(f["top_mag"][0]) == u32(f["top_mag"][1]) and not f["shortcut"], name      # the float values tie too
        if "shortcut" in w:
            assert f["shortcut"] == w["shortcut"], name
        if w.get("one_lane_at_8"):
            # every tie of the integer stage sits in one lane, and the one at the eighth candidate is cut in two
            m8 = f["mag1"][f["cand"][7]]
            grp = [int(i) for i in np.flatnonzero(f["mag1"] == m8)]
            assert len({lane_of(i) for i in grp}) == 1 and 0 < len(set(grp) & set(f["cand"])) < len(grp), (name, grp, f["cand"])
            assert set(grp) & set(f["top"]), (name, grp, f["top"])
        if "n_valid" in w:
            valid = [i for i in f["top"] if i >= 0]
            assert len(valid) == w["n_valid"] and -1 in f["top"] and w["valid_at"] in valid and w["valid_at"] in (62, 63, 64), (name, f["top"])
            assert len(f["cand"]) == 8 and np.isinf(f["mag"][valid]).all() and np.isnan(f["mag"][[c for c in f["cand"] if c not in valid]]).all(), name
        if "cfo_near" in w:
            # the preamble rows: the fine CFO is the LTS part's extra rotation, wrapped into (-pi/64, pi/64], next to its edge
            wrapped = (w["cfo_near"] + np.pi / 64) % (np.pi / 32) - np.pi / 64
            assert abs(float(f["cfo_fine"]) - wrapped) < 1e-5, (name, f["cfo_fine"], wrapped)
        if f["found"]:
            # a ZERO Im gives cfo_fine = -0 nowhere (tests/lts_rows.py): no peak value has a -0 part, Im = -0 only beside Re < 0
            lo, hi = f["frame_start"], f["frame_start"] + f["found"]
            z = np.array([f["corr_re"][lo], f["corr_im"][lo], f["corr_re"][hi], f["corr_im"][hi]], np.float32)
            assert not (u32(z) == 0x80000000).any(), name
            assert not (u32(f["pi"])[0] == 0x80000000 and f["pr"] > 0), name
            if u32(f["cfo_fine"])[0] == 0x80000000:        # -0 all the same: a negative Im under a real part that overflowed to +Inf
                assert f["pi"] < 0 and np.isinf(f["pr"]) and w.get("minus_zero"), name
                args.add("-0")
        if w.get("sync"):
            assert f["flags"] & ref.F_SYNC, name
        if "found" in w:
            assert f["found"] == w["found"], (name, f["found"], f["top"])
        if "fs" in w:
            assert f["frame_start"] == w["fs"], (name, f["frame_start"])
        if "t" in w:
            assert f["t"] == w["t"], name
        if "arg" in w:
            want = np.float32(0) if w["arg"] == 0 else np.float32(np.sign(w["arg"])) * (PI if abs(w["arg"]) == 1 else np.float32(np.pi / 2)) / np.float32(w["found"])
            assert u32(f["cfo_fine"]) == u32(want), (name, f["cfo_fine"], want)
            assert f["corr_im"][w["fs"]] == 0 and u32(f["corr_im"][w["fs"]]) == 0, name
            args.add((w["found"], float(w["arg"])))
        if w.get("pi_abs"):
            assert abs(f["cfo_fine"]) == PI / np.float32(64), name
        q, v = f["q"], f["rint"]
        if w.get("rint128"):
            assert ((v == 128) & (q == 127)).any() and ((v == -128) & (q == -127)).any(), name
        if w.get("halves"):
            A = np.stack([f["yr"], f["yi"]], axis=1).reshape(-1) * f["scale"]
            half = np.abs(A - np.trunc(A)) == 0.5
            assert half.sum() >= 100 and (np.rint(A[half]) % 2 == 0).all(), name
        if w.get("burst_q0"):
            assert not q[:34].any() and (f["xr"][:17] != 0).sum() > 10 and f["E"] > 250, name
        if w.get("E255"):
            assert f["E"] == 255 and f["scale"] == np.float32(2.0 ** -122), name
        if w.get("inf_key"):
            assert np.isinf(f["top_mag"][:2]).all() and f["top_mag"][0] > 0, name
        seen["short" if f["shortcut"] else "wide"] += r["cls"] == "shortcut"
        if r["cls"] == "shortcut" and not f["shortcut"]:
            seen["wide_other_pair"] += record(restated(orc, r, ("shortcut_always",))) != record(f)
        founds.add(f["found"])
    assert seen["short"] >= 2 and seen["wide"] >= 2 and seen["wide_other_pair"] >= 1, seen
    assert founds == {0, 63, 64, 65}
    assert args == {(d, a) for d in (64, 65) for a in (0.0, 1.0, -1.0, 0.5, -0.5)} | {"-0"}, args
    # the closest ratios of the search: the third value a hair below / at or above 0.875f times the second
    for k, (g, h) in rows.SHORTCUT_GAINS.items():
        ratio = rows._shortcut_ratio(g, h)
        assert (0.95 < ratio < 1) if k == "below" else (1 <= ratio < 1.05), (k, ratio)
    # the rows' first candidates lie in at least 12 different lanes of the layout and in all three tiles (lag // 128)
    first = {f["cand"][0] for f in (restated(orc, r) for r in rows.table()) if f["L"] >= 383}
    assert len({lane_of(i) for i in first}) >= 12 and {i // 128 for i in first} == {0, 1, 2}


def test_recorded_shortcut_gains_are_the_closest_of_the_search():
    best = rows.search_shortcut_gains()
    assert {k: v[0] for k, v in best.items()} == rows.SHORTCUT_GAINS, best


def test_what_the_api_cannot_reach(orc):
    """t = 15 and the clamp of the scale field (see tests/lts_rows.py)"""
    import detect_rows as dr
    lts = rows.lts_c64()
    # the earliest trigger of any slot: a burst from sample 0, threshold 0, min_plateau 0
    x = np.concatenate([dr.ints_burst(40, 0, 3), np.zeros(400, np.complex64)])
    assert detect_ref.detect(x, 0.0, 0, first_only=True)[0].tolist() == [16]
    # the scale field is 260 - E: the clamp needs E < 6.  The smallest power-of-two burst that still triggers (thr 0:
    # wherever |A|^2 > 0) leaves E far above that
    smallest = None
    for e in range(-20, -80, -1):
        b = (dr.ints_burst(200, 0, 3) * np.float32(2.0 ** e)).astype(np.complex64)
        if len(detect_ref.detect(np.concatenate([b, np.zeros(300, np.complex64)]), 0.0, 0, first_only=True)[0]):
            smallest = e
    E = int(((np.abs(dr.ints_burst(16, 0, 3).real).max() * np.float32(2.0 ** smallest)).view(np.uint32) >> 23) & 0xff)
    assert smallest > -80 and 260 - E < 254 - 60, (smallest, E)


# mutant of the reference -> the row whose record it must change (profiles/lts_rows_mutations.txt says why)
MUTANTS = {
    "stage1_tie_high": "ties/p32/11",
    "top4_tie_high": "ties/lts64/20",
    "shortcut_always": "shortcut/near/22",
    "no_63_65": "pair/63",
    "last_pair_wins": "pair/64first",
    "nan_is_peak": "q8/nan_displaces",
    "clamp_128_wrap": "q8/round128",
    "nan_to_127": "q8/nan_displaces",
    "zero_383_before_max": "q8/sample383/0",
    "divide_by_64": "pair/65",
    "wave_min_is_max": "ties/p32rise/11",
    "lane_last_slot": "ties/lane8/47",
}


@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_reference_mutants_change_a_named_row(orc, mutant):
    by = {r["name"]: r for r in rows.table()}
    changed = [r["name"] for r in rows.table() if record(restated(orc, r, (mutant,))) != record(restated(orc, r))]
    txt = open(os.path.join(ROOT, "profiles", "lts_rows_mutations.txt")).read()
    assert mutant in txt
    if mutant == "shortcut_never":
        # the shortcut is an optimisation: the wide path must give the same record on every row
        assert changed == []
        return
    name = MUTANTS[mutant]
    assert name in changed and name in by, (mutant, changed)
    assert name in txt
