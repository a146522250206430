"""The host-made records and LLR rows of tests/soft_rows.py, on the CPU: every batch tests/test_gpu_soft_rows.py sends to
the device meets, in the reference alone, the conditions that keep it from passing vacuously (same table, same seeds);
the reference (tests/soft_viterbi_ref.py) decodes what a deliberately plain restatement of NUMERICS.md rule 14 decodes --
scalars, explicit loops over the 64 states, `<` and nothing else to compare -- for every value class, the non-finite and
the overflowing ones included; and `records` writes what a real demodulation writes in the fields the decoders read."""
import math

import numpy as np
import pytest

import soft_rows as sr
import soft_viterbi_ref as ref
from helpers import make_slots
from wifirx import txgen


def test_frame_dtype_is_the_bindings():
    from wifirx import capi
    assert sr.FRAME_DTYPE == capi.FRAME_DTYPE
    assert (sr.F_DETECTED, sr.F_SYNC, sr.F_SIGNAL, ref.F_COMPLETE, ref.F_LLR) == \
        (capi.F_DETECTED, capi.F_SYNC, capi.F_SIGNAL, capi.F_COMPLETE, capi.F_LLR)


def test_the_table_covers_what_the_issue_lists():
    assert set(sr.VALUE_SPECS + sr.LONG_SPECS + sr.SHAPE_SPECS + sr.LLR_BITS_SPECS + sr.TASK_SPECS + sr.GEOMETRY_SPECS) == set(sr.SPECS)
    assert {sr.SPECS[s].cls for s in sr.VALUE_SPECS} == set(sr.VALUE_CLASSES)
    for s in sr.VALUE_SPECS:
        enc, ln, _ = sr.SPECS[s].layout[0](*sr.SPECS[s].layout[1])
        assert enc.size >= 300 and all(len(set(ln[enc == e].tolist())) >= 3 for e in range(8))
    assert {sr.SPECS[s].llr_bits for s in sr.LLR_BITS_SPECS} == {1, 2, 4, 6}


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", sorted(sr.SPECS))
def test_batch_conditions_hold_in_the_reference(name, fmt):
    fig = sr.check_conditions(name, fmt)
    print(name, fmt, fig)


@pytest.mark.parametrize("name", sr.TASK_SPECS)
def test_task_batches_hold_enough_tasks(name):
    """sixteen tasks, four per bits-per-carrier class, two per rate: at most three waves then serve >= 4 tasks each, and a
    wave of a class's launch takes a second task of the class's other rate"""
    b = sr.build(name, "f32")
    n_tasks, longest = sr.n_tasks_and_longest(b)
    assert n_tasks == 16 and n_tasks >= 4 * 3
    assert longest == int((b.recs["n_sym"].astype(np.int64) * np.array(ref.N_DBPS)[b.recs["encoding"]]).max())


# ---- rule 14 once more, as plainly as it can be said ----

F32 = np.float32


def plain_coded_stream(row, enc, psdu_len):
    """the de-punctured coded stream of one frame: the transmitter's puncturing and interleaver (txgen) run backwards"""
    n_bpsc, n_cbps, n_dbps, _, rate = txgen.RATE_TABLE[enc]
    n_sym = int(math.ceil((16 + 8 * psdu_len + 6) / n_dbps))
    j = txgen.interleaver_map(n_cbps, n_bpsc)
    out = []
    for q in range(n_sym):
        k = 0
        for ci in range(2 * n_dbps):
            if (rate == "2/3" and ci % 4 == 3) or (rate == "3/4" and ci % 6 in (3, 4)):
                out.append(F32(0))
                continue
            v = F32(row[q * n_cbps + int(j[k])])
            k += 1
            out.append(v if math.isfinite(float(v)) else F32(0))
    return out


def plain_viterbi(coded):
    """NUMERICS.md rule 14 for one frame, float32 scalars; returns (decoded bits, whether the metrics ended as NaN)"""
    n = len(coded) // 2
    inf = F32(np.inf)
    pm = [F32(0)] + [inf] * 63
    surv = []

    def expected(p, bit):
        r = (p << 1) | bit                                   # bit k of r = the input delayed by k steps
        a = (r ^ (r >> 2) ^ (r >> 3) ^ (r >> 5) ^ (r >> 6)) & 1          # 133 octal
        b = (r ^ (r >> 1) ^ (r >> 2) ^ (r >> 3) ^ (r >> 6)) & 1          # 171 octal
        return a, b

    for t in range(n):
        if t > 0 and t % 24 == 0:
            mn = pm[0]
            for s in range(1, 64):
                if pm[s] < mn:
                    mn = pm[s]
            pm = [F32(v - mn) for v in pm]
        la, lb = coded[2 * t], coded[2 * t + 1]
        cost_a = (la if la > 0 else F32(0), -la if -la > 0 else F32(0))          # cost of expecting 0, of expecting 1
        cost_b = (lb if lb > 0 else F32(0), -lb if -lb > 0 else F32(0))
        new, bits = [], []
        for s in range(64):
            p0 = s >> 1
            p1 = p0 | 32
            a0, b0 = expected(p0, s & 1)
            a1, b1 = expected(p1, s & 1)
            m0 = F32(pm[p0] + F32(cost_a[a0] + cost_b[b0]))
            m1 = F32(pm[p1] + F32(cost_a[a1] + cost_b[b1]))
            if m1 < m0:
                new.append(m1)
                bits.append(1)
            else:
                new.append(m0)
                bits.append(0)
        pm = new
        surv.append(bits)
    best = 0
    for s in range(1, 64):
        if pm[s] < pm[best]:
            best = s
    n_nan = sum(1 for v in pm if v != v)
    assert n_nan in (0, 64)
    out = [0] * n
    s = best
    for t in range(n - 1, -1, -1):
        out[t] = s & 1
        s = (s >> 1) | (surv[t][s] << 5)
    return np.array(out, np.uint8), n_nan == 64


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", sr.VALUE_SPECS)
def test_reference_equals_the_plain_restatement(name, fmt):
    b, fr, psdu, nan = sr.reference(name, fmt)
    ln = b.recs["psdu_len"]
    short = np.nonzero(ln == ln.min())[0] if name != "values_const_random" else np.arange(b.recs.size)
    pick = [int(short[short % 8 == e][0]) for e in (0, 3, 5, 6)]          # one frame per bits-per-carrier class, all three puncturings
    if nan.any():
        pick += [int(np.nonzero(nan)[0][0]), int(np.nonzero(nan)[0][-1]), int(np.nonzero(~nan)[0][0])]
    with np.errstate(all="ignore"):
        for k in pick:
            enc, l = int(b.recs["encoding"][k]), int(ln[k])
            coded = plain_coded_stream(b.rows_f32[k], enc, l)
            want = ref.coded_llrs(b.rows_f32[k:k + 1], enc, l)
            assert np.array_equal(np.array(coded, np.float32).view(np.uint32), want[0].view(np.uint32)), (name, k)
            bits, ended_nan = plain_viterbi(coded)
            assert len(bits) <= 700
            assert np.array_equal(bits, ref.viterbi_soft(want)[0]), (name, k)
            assert ended_nan == bool(nan[k])
            by, ok = ref.finish(bits[None, :], l)
            assert np.array_equal(by[0], psdu[k, :l]) and bool(ok[0]) == bool(fr["flags"][k] & ref.F_CRC_OK)


def test_overflow_regime_is_defined_not_an_exception():
    """rows of magnitude 1e38 with a tenth of the signs wrong: all 64 metrics reach +inf between two normalisations, become
    NaN there, and the frame decodes to what no comparison being true gives -- survivor bits and end state 0"""
    recs = sr.records([2] * 4, 40)
    signs, _ = sr.coherent(recs, int(recs["n_sym"][0]), 2, seed=3)
    rng = np.random.default_rng(4)
    x = (signs * np.where(rng.random(signs.shape) < 0.1, -1, 1) * np.float32(1e38)).astype(np.float32)
    nan = np.zeros(4, bool)
    fr, psdu = ref.decode_batch(recs, x, int(recs["n_sym"][0]), psdu_stride=64, llr_bits=2, nan_out=nan)
    assert nan.all() and ((fr["flags"] & ref.F_DECODED) != 0).all()
    dec = ref.viterbi_soft(ref.coded_llrs(x, 2, 40))
    t_nan = [plain_first_nan_step(ref.coded_llrs(x[k:k + 1], 2, 40)[0]) for k in range(4)]
    for k in range(4):
        assert t_nan[k] is not None and t_nan[k] % 24 == 0
        assert not dec[k, t_nan[k]:].any()          # from the NaN step on: state 0 traced back through zero survivor bits


def plain_first_nan_step(coded):
    """the step before which the normalisation first found all 64 metrics at +inf, by the reference's own arithmetic"""
    pm = np.full(64, np.inf, np.float32)
    pm[0] = 0
    with np.errstate(all="ignore"):
        for t in range(coded.size // 2):
            if t and t % 24 == 0:
                if np.isinf(pm.min()):
                    return t
                pm = pm - pm.min()
            la, lb = coded[2 * t], coded[2 * t + 1]
            ca = (max(la, np.float32(0)), max(-la, np.float32(0)))
            cb = (max(lb, np.float32(0)), max(-lb, np.float32(0)))
            bm = np.array([ca[0] + cb[0], ca[0] + cb[1], ca[1] + cb[0], ca[1] + cb[1]], np.float32)
            m0 = pm[ref._P0] + bm[ref._AB0]
            m1 = pm[ref._P1] + bm[ref._AB1]
            pm = np.where(m1 < m0, m1, m0)
    return None


# ---- the records helper against a real demodulation ----

@pytest.mark.parametrize("enc", range(8))
def test_records_equal_a_demodulated_batch(orc, enc):
    plen = 40 + 37 * enc
    iq, slot_len, tx = make_slots(12, enc, psdu_len=plen, snr_db=28.0, seed=60 + enc)
    o = orc.demod_batch(iq, slot_len, orc.make_params(max_sym=tx.n_sym, llr_bits=6))
    got, want = sr.records(enc, [plen] * 12), o["frames"]
    both = ref.F_COMPLETE | ref.F_LLR
    assert ((want["flags"] & both) == both).all()
    assert np.array_equal(got["flags"] & both, want["flags"] & both)
    assert np.array_equal(got["flags"], want["flags"])          # and the other flags of a complete frame
    for f in ("encoding", "psdu_len", "n_sym", "n_sym_out", "n_bpsc"):
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(ref.decodable(got, tx.n_sym, 2048), ref.decodable(want, tx.n_sym, 2048))
