"""The symbol path on host-built slots, CPU part: the restatement of tests/symbol_ref.py (NUMERICS.md rules 7, 7a, 12, 15)
against the oracle on every row of tests/symbol_rows.py -- the record from the constructed SIGNAL bits; the decisions, the
LLRs (llr_csi 0 and 1) and the bit planes from the oracle's own equalised points --, the oracle's Viterbi and the packed
model of tests/test_signal_viterbi_packed.py on the words far from every codeword, the table's conditions asserted on the
references alone, and the mutants of the restatement, each of which must change named rows."""
import os
import re

import numpy as np
import pytest

import symbol_ref as ref
import symbol_rows as rows
from helpers import planes_of
from test_signal_viterbi_packed import packed_viterbi4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQS = (0, 1, 2, 3)
EQ_NAMES = ("LS", "LMS", "COMB", "STA")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """float32 arrays: NaN by position, every other value by its bits (-0 differs from +0)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and np.array_equal(u32(got)[~ng], u32(want)[~nw])


def test_thresholds_are_the_tables_bit_for_bit():
    txt = open(os.path.join(ROOT, "include", "wifirx_tables.h")).read()
    for name, v in ref.THRESHOLDS.items():
        m = re.search(r"#define %s (\S+?)f?\s" % name, txt)
        assert np.float32(float.fromhex(m.group(1))) == v and float(np.float32(float.fromhex(m.group(1)))) == float.fromhex(m.group(1)), name
    for name, v in (("WR_LEVEL_16QAM", ref.A16), ("WR_LEVEL_64QAM", ref.A64)):
        m = re.search(r"#define %s (\S+?)f?\s" % name, txt)
        assert np.float32(float.fromhex(m.group(1))) == v, name


def group_out(orc, grp, chan_est, llr_csi=0):
    return [rows.expected(orc, r, "v", chan_est, llr_csi) for r in rows.group(grp)]


@pytest.mark.parametrize("chan_est", EQS)
def test_records_from_the_constructed_bits(orc, chan_est):
    """flags (SIGNAL, LLR, TRUNCATED, COMPLETE), encoding, psdu_len, n_bpsc, n_sym, n_sym_out of every row: the oracle
    against the restatement's Viterbi, parser and bookkeeping on the 48 bits the row was built from"""
    for grp, g in rows.GROUPS.items():
        for r, o in zip(rows.group(grp), group_out(orc, grp, chan_est)):
            fr = o["frame"]
            assert fr["flags"] & orc.F_SYNC, r["name"]
            want = rows.restated_record(r, fr, rows.slot_of(r).size, g["max_sym"])
            assert rows.record_tuple(fr) == rows.record_tuple(want), (r["name"], fr, want)


def points_values(o):
    """the float32 components of the n_sym_out written symbols' points of one oracle output"""
    e = o["eq"][:int(o["frame"]["n_sym_out"])]
    return np.concatenate([e.real.ravel(), e.imag.ravel()]).astype(np.float32)


@pytest.mark.parametrize("llr_csi", (0, 1))
@pytest.mark.parametrize("chan_est", EQS)
def test_slicer_and_llrs_from_the_oracles_points(orc, chan_est, llr_csi):
    """idx, the LLRs and the bit planes of every row with data symbols: rule 7 (and 12) applied to the oracle's own `eq`"""
    for grp, g in rows.GROUPS.items():
        ms = g["max_sym"]
        for r, o in zip(rows.group(grp), group_out(orc, grp, chan_est, llr_csi)):
            fr = o["frame"]
            n, nb = int(fr["n_sym_out"]), int(fr["n_bpsc"])
            if not n:
                continue
            Y = o["eq"][:n]
            idx = ref.decide(Y, nb)
            assert np.array_equal(idx, o["idx"][:n]), r["name"]
            want = ref.llr_weighted(Y, nb, ref.weight(o["csi"])) if llr_csi else ref.llr(Y, nb)
            assert fr["flags"] & orc.F_LLR
            assert same_bits(o["llr"][:n * 48 * nb], want.reshape(-1)), r["name"]
            recs = np.array([fr], dtype=orc.FRAME_DTYPE)
            assert np.array_equal(ref.planes(idx, nb, n, ms), planes_of(recs, o["idx"][None], ms)[0]), r["name"]
            # rule 15: the bf16 pattern keeps the sign and the zero of every LLR (a point ON a threshold has LLR +0)
            b = ref.llr_bf16(want.reshape(-1))
            f = want.reshape(-1)
            ok = ~np.isnan(f)
            assert np.array_equal((b[ok] >> 15) == 1, np.signbit(f[ok])) and np.array_equal((b[ok] & 0x7fff) == 0, f[ok] == 0), r["name"]


def test_oracle_viterbi_on_words_far_from_every_codeword(orc):
    """orc.viterbi and orc.decode_signal against the scalar Viterbi of the restatement"""
    for r in rows.group("sig"):
        de = ref.deinterleave(r["sig48"])
        bits, info = ref.viterbi24(de)
        assert list(orc.viterbi(np.array(de, np.uint8), 24)) == bits, r["name"]
        ok, enc, ln = orc.decode_signal(r["sig48"])
        want = ref.decode_signal(r["sig48"])
        assert (ok, enc if ok else 0, ln if ok else 0) == want, r["name"]


def test_packed_model_on_the_same_words():
    """four DIFFERENT words in the four bytes of a register, every word in every byte.  The largest byte the model reaches
    on this table is 67: the start value 64 of an unreachable state plus the branch metrics of the first steps (all 64
    states are reached after six steps, and from then on no metric exceeds SEARCHED["top"] = 13)"""
    R = rows.group("sig")
    worst = 0
    for rot in range(4):
        order = R[rot:] + R[:rot]
        order = order + order[:(-len(order)) % 4]
        for k in range(0, len(order), 4):
            four = order[k:k + 4]
            cbs = [rows.bits_word(ref.deinterleave(r["sig48"])) for r in four]
            got, top = packed_viterbi4(cbs)
            worst = max(worst, top)
            for f, r in enumerate(four):
                assert [(got[f] >> t) & 1 for t in range(24)] == ref.viterbi24(ref.deinterleave(r["sig48"]))[0], r["name"]
    print("largest packed metric byte:", worst)
    assert worst < 128 and worst == PACKED_WORST


def test_what_the_unreachable_start_value_has_to_exceed():
    """A state reached at step t < 6 has a metric of at most 2 (t + 1) <= 12, after six steps every state is reached: any
    start value above 12 orders every comparison as 64 does (32 is asserted on every word of the table: a kernel with
    0x20202020 is the same decoder, which is why no row can tell it from 0x40404040), and a value the reachable metrics
    overtake does not (4: some word of the table decodes differently)"""
    R = rows.group("sig")
    R = R + R[:(-len(R)) % 4]
    differs = 0
    for k in range(0, len(R), 4):
        cbs = [rows.bits_word(ref.deinterleave(r["sig48"])) for r in R[k:k + 4]]
        want = packed_viterbi4(cbs)[0]
        assert packed_viterbi4(cbs, 0x20202020)[0] == want
        assert packed_viterbi4(cbs, 0x0d0d0d0d)[0] == want
        differs += packed_viterbi4(cbs, 0x04040404)[0] != want
    assert differs


PACKED_WORST = 67           # recorded: the maximum the model reaches on the table


def test_searched_words_are_what_the_file_says():
    by = rows.by_name()
    w, ends = rows.SEARCHED["tie0"]
    info = ref.viterbi24(ref.deinterleave(rows.word_bits(w)))[1]
    assert tuple(info["ends"]) == tuple(ends) and ends[0] == 0 and len(ends) > 1
    w, n = rows.SEARCHED["path"]
    assert ref.viterbi24(ref.deinterleave(rows.word_bits(w)))[1]["path_ties"] == n >= 6
    w, top = rows.SEARCHED["top"]
    assert ref.viterbi24(ref.deinterleave(rows.word_bits(w)))[1]["top"] == top
    assert top == max(ref.viterbi24(ref.deinterleave(r["sig48"]))[1]["top"] for r in rows.group("sig"))
    for k in ("tie0", "path"):                  # both parse: what the other rule would do shows in the record
        assert ref.decode_signal(by["far/searched/" + k]["sig48"])[0]


def ulps_from(v, T):
    return np.abs(v).view(np.int32).astype(np.int64) - int(np.float32(T).view(np.int32))


def test_table_conditions(orc):
    """section by section what tests/symbol_rows.py promises, on the references alone: a failure here means the table is
    wrong, not the device"""
    from independent_rx import IndependentRx
    by = rows.by_name()
    S = rows.group("sig")
    # every SIGNAL row's 48 decisions are the constructed bits: the independent receiver's SIGNAL points
    g = rows.GROUPS["sig"]
    ind = IndependentRx().receive(np.stack([rows.slot_of(r, g["slot"]) for r in S]), max_sym=g["max_sym"])
    assert ind["sync"].all()
    ys = ind["eq_signal"].real
    assert (np.abs(ys) > 0.5).all()
    assert np.array_equal((ys > 0).astype(np.uint8), np.stack([r["sig48"] for r in S]))
    for k, r in enumerate(S):
        ok, enc, ln = ref.decode_signal(r["sig48"])
        assert (bool(ind["signal_ok"][k]), int(ind["encoding"][k]) if ok else 0, int(ind["psdu_len"][k]) if ok else 0) == (ok, enc, ln), r["name"]
    # the random words: at least 40 parse, at least 100 do not, every encoding occurs
    rnd = [ref.decode_signal(r["sig48"]) for r in S if r["want"].get("random")]
    assert len(rnd) >= 200 and sum(d[0] for d in rnd) >= 40 and sum(not d[0] for d in rnd) >= 100
    assert {d[1] for d in rnd if d[0]} == set(range(8))
    # the field rows are what their names say
    for r in S:
        w = r["want"]
        if "ok" in w:
            assert ref.decode_signal(r["sig48"])[0] == w["ok"], r["name"]
        if "length" in w:
            assert ref.decode_signal(r["sig48"])[2] == w["length"], r["name"]
        bits = ref.viterbi24(ref.deinterleave(r["sig48"]))[0]
        if w.get("reserved"):
            assert bits[4] == 1
        if w.get("tail"):
            assert any(bits[18:])
    for k in range(16):
        assert ref.viterbi24(ref.deinterleave(by["field/rate%d" % k]["sig48"]))[0][0:4] == [(k >> i) & 1 for i in range(4)]
    # the n_sym step rows differ by one symbol, and one step per rate is max_sym | max_sym + 1
    for e in range(8):
        for n in (g["max_sym"], 40 + e):
            lo, hi = by["field/step%d/enc%d/lo" % (n, e)], by["field/step%d/enc%d/hi" % (n, e)]
            dl, dh = ref.decode_signal(lo["sig48"]), ref.decode_signal(hi["sig48"])
            assert dl[1] == dh[1] == e and dh[2] == dl[2] + 1
            assert (ref.n_sym_of(e, dl[2]), ref.n_sym_of(e, dh[2])) == (n, n + 1)
            fl, fh = (rows.expected(orc, r, "v")["frame"] for r in (lo, hi))
            assert (int(fl["n_sym"]), int(fh["n_sym"])) == (n, n + 1)
            if n == g["max_sym"]:
                assert fl["flags"] & orc.F_COMPLETE and not fh["flags"] & orc.F_COMPLETE and fh["flags"] & ref.F_TRUNCATED
    # the L rows differ in TRUNCATED
    for r in rows.group("end"):
        fr = rows.expected(orc, r, "v")["frame"]
        assert bool(fr["flags"] & ref.F_TRUNCATED) == r["want"]["truncated"] and int(fr["n_sym"]) == r["want"]["n_sym"], r["name"]
        assert bool(fr["flags"] & orc.F_COMPLETE) != r["want"]["truncated"]
    assert sum(r["want"]["truncated"] for r in rows.group("end")) >= 4 and sum(not r["want"]["truncated"] for r in rows.group("end")) >= 4
    # the claimed rates: all eight, all sliced with points made for 64-QAM
    assert [int(rows.expected(orc, by["claim/enc%d" % e], "v")["frame"]["encoding"]) for e in range(8)] == list(range(8))
    # exact zeros: the rows complete with every symbol written
    for r in rows.group("zero"):
        for ce in EQS:
            fr = rows.expected(orc, r, "v", ce)["frame"]
            assert fr["flags"] & orc.F_COMPLETE and fr["n_sym_out"] == rows.GROUPS["zero"]["max_sym"], r["name"]


# WR_T64_6 under LMS, COMB and STA: these three equalise by Y = (X conj(H)) r with r = sp_recip(|H|^2) (rule 11).  The clean
# preamble gives |H|^2 = 78.77, so a numerator of 6a |H|^2 = 72.9 lies in [64, 128), where neighbouring floats are 2^-17
# apart, while the quotient lies in [0.5, 1), where they are 2^-24 apart: consecutive numerators land 2^-17 / 78.77 = 1.6
# quotient ulps apart and the quotient skips more than a third of the floats around 6a.  For the few values of |H|^2 these
# rows have, WR_T64_6 itself is among the skipped ones (it is the nearest float of 6 / sqrt(42): nothing is wrong with the
# constant).  2a and 4a (numerators in [16, 32) and [32, 64), 0.8 ulps apart) and LS (Y = X G, rule 7) do not skip.
NO_EXACT = {("WR_T64_6", 1), ("WR_T64_6", 2), ("WR_T64_6", 3)}


@pytest.mark.parametrize("chan_est", EQS)
def test_points_lie_on_the_thresholds(orc, chan_est):
    """per equaliser and threshold: at least 20 components bit-equal to it and 20 on each neighbouring float (the named
    exception: 50 on each neighbour); BPSK and QPSK: +0, both signs below 1e-6, under STA a -0"""
    T = rows.group("thr") + rows.group("end") + rows.group("long")
    out = [rows.expected(orc, r, "v", chan_est) for r in T]

    def values(nb):
        return np.concatenate([points_values(o) for r, o in zip(T, out) if int(o["frame"]["n_bpsc"]) == nb and r["cls"] != "claim"])
    for name, thr in ref.THRESHOLDS.items():
        d = ulps_from(values(4 if name == "WR_T16_2" else 6), thr)
        counts = tuple(int((d == k).sum()) for k in (0, -1, 1))
        print(EQ_NAMES[chan_est], name, "equal / 1 ulp below / 1 ulp above:", counts)
        if (name, chan_est) in NO_EXACT:
            assert counts[0] == 0 and min(counts[1:]) >= 50, (name, counts)
        else:
            assert min(counts) >= 20, (name, counts)
    minus_zero = 0
    for nb in (1, 2):
        v = values(nb)
        pz, mz = int(((v == 0) & ~np.signbit(v)).sum()), int(((v == 0) & np.signbit(v)).sum())
        pos, neg = int(((v > 0) & (v < 1e-6)).sum()), int(((v < 0) & (v > -1e-6)).sum())
        print(EQ_NAMES[chan_est], "n_bpsc", nb, "+0 / -0 / small positive / small negative:", (pz, mz, pos, neg), "largest", float(np.abs(v).max()))
        assert pz >= 100 and pos >= 100 and neg >= 100, (nb, pz, pos, neg)
        minus_zero += mz
        if chan_est in (1, 3):
            assert np.abs(v).max() > 1.0            # the regime of sp_recip and of the update the long rows are there for
    if chan_est == 3:
        assert minus_zero >= 1


# ---- the mutants of the restatement -------------------------------------------------------------------------------------

def changed_records(orc, mut):
    out = set()
    for grp, g in rows.GROUPS.items():
        for r in rows.group(grp):
            fr = rows.expected(orc, r, "v")["frame"]
            n = rows.slot_of(r).size
            if rows.record_tuple(rows.restated_record(r, fr, n, g["max_sym"], (mut,))) != rows.record_tuple(rows.restated_record(r, fr, n, g["max_sym"])):
                out.add(r["name"])
    return out


def changed_decisions(orc, mut):
    out = set()
    for grp in rows.GROUPS:
        for r in rows.group(grp):
            o = rows.expected(orc, r, "v")
            n, nb = int(o["frame"]["n_sym_out"]), int(o["frame"]["n_bpsc"])
            if n and not np.array_equal(ref.decide(o["eq"][:n], nb, (mut,)), o["idx"][:n]):
                out.add(r["name"])
    return out


def test_mutants_of_the_restatement(orc):
    """each deliberate mistake changes the rows that were built against it (and the oracle, which equals the unmutated
    restatement on every row, differs from the mutant there)"""
    by = rows.by_name()
    ms = rows.GROUPS["sig"]["max_sym"]
    steps = {"field/step%d/enc%d/%s" % (n, e, s) for e in range(8) for n in (ms, 40 + e) for s in ("lo", "hi")}

    c = changed_records(orc, "m1_le_m0")
    assert "far/searched/path" in c and not any(n.startswith("field/") for n in c), sorted(c)[:8]
    c = changed_records(orc, "final_highest")
    assert "far/searched/tie0" in c and not any(n.startswith("field/") for n in c)
    c = changed_records(orc, "end_state_0")
    tails = {r["name"] for r in rows.group("sig") if r["want"].get("tail")}
    assert len([n for n in c if n.startswith("far/random/")]) >= 10
    # a codeword with non-zero tail bits ends in another state than 0: forcing 0 decodes another word
    assert tails & c
    c = changed_records(orc, "parity16")
    want = {r["name"] for r in table_all() if ref.viterbi24(ref.deinterleave(r["sig48"]))[0][16] == 1}
    assert {"field/len2048/enc0", "field/len4095/enc7"} <= c and c == {n for n in want if n in c} and len(c) >= 4
    c = changed_records(orc, "reserved_rejected")
    assert {"field/reserved/11", "field/reserved/9", "field/reserved/12", "field/reserved/len41"} <= c
    assert all(ref.viterbi24(ref.deinterleave(by[n]["sig48"]))[0][4] == 1 for n in c)
    c = changed_records(orc, "n_sym_floor")
    assert steps <= c
    c = changed_records(orc, "complete_minus1")
    short = {r["name"] for r in rows.group("end") if r["name"].endswith("short1")}
    assert short <= c and {"field/step%d/enc%d/hi" % (ms, e) for e in range(8)} <= c
    c = changed_records(orc, "fit_207")                 # one sample short counts as fitting: exactly the short1 rows
    assert c == short
    c = changed_decisions(orc, "re_ge_0")
    assert {r["name"] for r in rows.group("thr") if r["want"].get("nb") in (1, 2)} <= c
    assert not any(n.startswith("thr/nb4") or n.startswith("thr/nb6") for n in c)
    c = changed_decisions(orc, "abs_le_2a")
    assert {r["name"] for r in rows.group("thr") if r["want"].get("nb") == 4} <= c
    assert not any(n.startswith("thr/nb1") or n.startswith("thr/nb2") or n.startswith("thr/nb6") for n in c)
    assert set(ref.MUTANTS) == {"m1_le_m0", "final_highest", "end_state_0", "parity16", "reserved_rejected", "n_sym_floor",
                                "complete_minus1", "fit_207", "re_ge_0", "abs_le_2a"}


def table_all():
    return rows.table()
