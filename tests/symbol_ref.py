"""The decision rules of the symbol path, restated from the text alone (NUMERICS.md rules 7, 7a, 12, 15; SURVEY.md App.
A.5 (7), A.6, A.7; include/wifirx.h for the record and the bit planes): the SIGNAL chain from 48 hard decisions, the
data-symbol bookkeeping of a frame record, and the slicer with its LLRs as functions of a GIVEN float32 point Y.  Plain
NumPy and Python integers; nothing of the product or the oracle is imported (tests/llr_bf16_ref.py is NumPy alone).  The
float chain that leads to Y (the FFT and rules 8 to 11) is not restated here: the oracle (bit for bit) and
tests/independent_rx.py (float64) stay its references.

`mut` names ONE deliberate mistake at a time (MUTANTS); tests/test_symbol_rows.py asserts which rows of
tests/symbol_rows.py each of them changes."""
import numpy as np

from llr_bf16_ref import bf16_rne

F32 = np.float32

MUTANTS = ("m1_le_m0", "final_highest", "end_state_0", "parity16", "reserved_rejected", "n_sym_floor", "re_ge_0", "abs_le_2a",
           "complete_minus1", "fit_207")

F_SIGNAL, F_COMPLETE, F_LLR, F_TRUNCATED = 0x04, 0x08, 0x10, 0x80

# ---- rule 7: a and the thresholds, each ONE float32 product of a float32 integer and the float32 amplitude unit ---------
A16, A64 = F32(np.sqrt(1.0 / 10.0)), F32(np.sqrt(1.0 / 42.0))
T16_2 = F32(2) * A16
T64_2, T64_4, T64_6 = F32(2) * A64, F32(4) * A64, F32(6) * A64
THRESHOLDS = {"WR_T16_2": T16_2, "WR_T64_2": T64_2, "WR_T64_4": T64_4, "WR_T64_6": T64_6}

# 802.11 Table 18-6, RATE bits R1..R4 with R1 in bit 0 -> encoding; encoding -> N_BPSC, N_DBPS
RATE = {11: 0, 15: 1, 10: 2, 14: 3, 9: 4, 13: 5, 8: 6, 12: 7}
N_BPSC = (1, 1, 2, 2, 4, 4, 6, 6)
N_DBPS = (24, 36, 48, 72, 96, 144, 192, 216)

# data carrier c -> FFT bin in shifted order (bin 32 = DC; pilots at 11, 25, 39, 53), and its place among the 52 used bins
DATA_BINS = [i for i in range(6, 59) if i not in (11, 25, 32, 39, 53)]
USED_BINS = [i for i in range(6, 59) if i != 32]
DATA_IN_USED = [USED_BINS.index(i) for i in DATA_BINS]


def _par(v):
    return bin(v).count("1") & 1


def deinterleave(rx48):
    """deint[i] = rx[3 (i % 16) + i / 16]"""
    return [int(rx48[3 * (i % 16) + i // 16]) for i in range(48)]


def conv_encode(bits):
    """K = 7, generators 0155 / 0117 over (state << 1 | input), state = the six previous inputs, the newest in bit 0"""
    state, out = 0, []
    for b in bits:
        reg = (state << 1) | int(b)
        out += [_par(reg & 0o155), _par(reg & 0o117)]
        state = reg & 63
    return out


def interleave(coded48):
    """the transmitter's side of deinterleave(): the 48 bits in carrier order"""
    rx = [0] * 48
    for i in range(48):
        rx[3 * (i % 16) + i // 16] = int(coded48[i])
    return rx


_VITERBI_MUTANTS = ("m1_le_m0", "final_highest", "end_state_0")
_viterbi_cache = {}


def viterbi24(coded, mut=()):
    """viterbi24_scalar, each (word, mutant) computed once"""
    key = (tuple(int(c) for c in coded), tuple(m for m in _VITERBI_MUTANTS if m in mut))
    if key not in _viterbi_cache:
        _viterbi_cache[key] = viterbi24_scalar(key[0], key[1])
    bits, info = _viterbi_cache[key]
    return list(bits), dict(info)


def viterbi24_scalar(coded, mut=()):
    """Scalar 64-state Viterbi over 24 steps on 48 hard bits (A0 B0 A1 B1 ...).  State s after a step = the six newest
    inputs, the newest in bit 0; its predecessors are s >> 1 (candidate 0) and (s >> 1) | 32 (candidate 1), the branch bits
    the generators over ((predecessor << 1) | newest).  Start: state 0 at metric 0, every other state unreachable.
    Candidate 1 survives only if strictly smaller.  End: the lowest state among the smallest metrics (the end state is NOT
    forced to 0).  Returns (the 24 decoded bits, info): info = final metrics, end state, the number of tied
    add-compare-selects on the surviving path, the largest REACHABLE metric over all steps."""
    BIG = 1 << 20
    pm = [BIG] * 64
    pm[0] = 0
    dec, tie, top = [], [], 0
    for t in range(24):
        ra, rb = int(coded[2 * t]), int(coded[2 * t + 1])
        nm, d, ti = [0] * 64, [0] * 64, [False] * 64
        for s in range(64):
            p0, p1 = s >> 1, (s >> 1) | 32
            f0, f1 = (p0 << 1) | (s & 1), (p1 << 1) | (s & 1)
            m0 = pm[p0] + (ra != _par(f0 & 0o155)) + (rb != _par(f0 & 0o117))
            m1 = pm[p1] + (ra != _par(f1 & 0o155)) + (rb != _par(f1 & 0o117))
            take1 = m1 <= m0 if "m1_le_m0" in mut else m1 < m0
            nm[s], d[s] = (m1, 1) if take1 else (m0, 0)
            ti[s] = m0 == m1 and m0 < BIG
        pm = nm
        dec.append(d)
        tie.append(ti)
        top = max([top] + [m for m in pm if m < BIG])
    best = min(pm)
    ends = [s for s in range(64) if pm[s] == best]
    st = 0 if "end_state_0" in mut else ends[-1] if "final_highest" in mut else ends[0]
    info = dict(final=list(pm), end=st, ends=ends, top=top)
    bits, ties = [0] * 24, 0
    for t in range(23, -1, -1):
        bits[t] = st & 1
        ties += tie[t][st]
        st = (st >> 1) | (dec[t][st] << 5)
    info["path_ties"] = ties
    return bits, info


def parse(bits, mut=()):
    """24 decoded bits -> (ok, encoding, length): even parity over bits 0..16 against bit 17, RATE = bits 0..3, LENGTH = bits
    5..16 (LSB first); bit 4 (reserved) and bits 18..23 (tail) are ignored"""
    n_par = 16 if "parity16" in mut else 17
    if sum(bits[:n_par]) & 1 != bits[17]:
        return False, 0, 0
    if "reserved_rejected" in mut and bits[4]:
        return False, 0, 0
    r = bits[0] | bits[1] << 1 | bits[2] << 2 | bits[3] << 3
    if r not in RATE:
        return False, 0, 0
    return True, RATE[r], sum(bits[5 + i] << i for i in range(12))


def decode_signal(rx48, mut=()):
    """48 hard decisions in carrier order -> (ok, encoding, length)"""
    return parse(viterbi24(deinterleave(rx48), mut)[0], mut)


def n_sym_of(enc, length, mut=()):
    n = 16 + 8 * length + 6
    return n // N_DBPS[enc] if "n_sym_floor" in mut else -(-n // N_DBPS[enc])


def record(rx48, L, frame_start, max_sym, llr_bits, mut=()):
    """What a frame that synchronised at `frame_start` with L copied samples and these 48 SIGNAL decisions puts into its
    record.  Symbol s (0, 1: the long training symbols, 2: SIGNAL, 3 + q: data symbol q) reads the 64 samples from
    frame_start + 64 s (s < 2) or frame_start + 144 + 80 (s - 2) on; a symbol that does not lie within L, or a data symbol
    q >= max_sym, ends the frame as TRUNCATED.  COMPLETE: every one of the n_sym data symbols was written."""
    out = dict(flags=0, encoding=0, psdu_len=0, n_bpsc=0, n_sym=0, n_sym_out=0)
    if frame_start + 144 + 64 > L:
        out["flags"] = F_TRUNCATED
        return out
    ok, enc, length = decode_signal(rx48, mut)
    if not ok:
        return out
    n_sym = n_sym_of(enc, length, mut)
    fit = (L - frame_start - (207 if "fit_207" in mut else 208)) // 80      # data symbols whose 64 samples end at or before L
    n_out = min(n_sym, max_sym, fit)
    flags = F_SIGNAL | (F_LLR if llr_bits and N_BPSC[enc] <= llr_bits else 0)
    if n_out < n_sym:
        flags |= F_TRUNCATED
    if (n_out >= n_sym - 1) if "complete_minus1" in mut else (n_out == n_sym):
        flags |= F_COMPLETE
    out.update(flags=flags, encoding=enc, psdu_len=length, n_bpsc=N_BPSC[enc], n_sym=n_sym, n_sym_out=n_out)
    return out


# ---- rule 7: slicer and LLRs of given float32 points -------------------------------------------------------------------

def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def decide(Y, n_bpsc, mut=()):
    """index of a point (LSB = first transmitted bit): every comparison is strict, so a component EQUAL to a threshold
    decides 0 for that bit, and +0 as well as -0 decide `not positive` (rule 7a).  NaN compares false throughout."""
    Y = np.asarray(Y, dtype=np.complex64)
    re, im = _f32(Y.real), _f32(Y.imag)
    are, aim = np.abs(re), np.abs(im)
    pos = (lambda u: u >= 0) if "re_ge_0" in mut else (lambda u: u > 0)
    lt2 = (lambda u, t: u <= t) if "abs_le_2a" in mut else (lambda u, t: u < t)
    with np.errstate(invalid="ignore"):
        if n_bpsc == 1:
            r = pos(re) * 1
        elif n_bpsc == 2:
            r = pos(re) * 1 | pos(im) * 2
        elif n_bpsc == 4:
            r = pos(re) * 1 | lt2(are, T16_2) * 2 | pos(im) * 4 | lt2(aim, T16_2) * 8
        else:
            r = (pos(re) * 1 | (are < T64_4) * 2 | ((are < T64_6) & (are > T64_2)) * 4 |
                 pos(im) * 8 | (aim < T64_4) * 16 | ((aim < T64_6) & (aim > T64_2)) * 32)
    return np.asarray(r).astype(np.uint8)


def llr(Y, n_bpsc):
    """[..., n_bpsc] float32: per axis u, L0 = u, L1 = 2a - |u| (16-QAM); L0 = u, L1 = 4a - |u|, L2 = 2a - ||u| - 4a|
    (64-QAM); the bits of the real axis first; each difference ONE float32 subtraction"""
    Y = np.asarray(Y, dtype=np.complex64)
    re, im = _f32(Y.real), _f32(Y.imag)

    def axis(u):
        if n_bpsc <= 2:
            return [u]
        if n_bpsc == 4:
            return [u, T16_2 - np.abs(u)]
        return [u, T64_4 - np.abs(u), T64_2 - np.abs(np.abs(u) - T64_4)]
    with np.errstate(invalid="ignore"):
        parts = axis(re) + (axis(im) if n_bpsc > 1 else [])
    return np.stack(parts, axis=-1).astype(np.float32)


def weight(csi52):
    """rule 12: w = fma(H.im, H.im, H.re^2) of the LS estimate on the 52 used bins -> the 48 data carriers' weights.  The
    square H.re^2 is a float32 product (rounded), the fma rounds once: formed here in float64 -- H.im^2 is exact there --
    with the sum rounded to odd (TwoSum's error decides), so that the second rounding to float32 cannot fall on a tie."""
    H = np.asarray(csi52, dtype=np.complex64)[..., DATA_IN_USED]
    im = _f32(H.imag).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        a = im * im
        b = (_f32(H.real) * _f32(H.real)).astype(np.float64)
        s = a + b
        bv = s - a
        e = (a - (s - bv)) + (b - bv)
        fix = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def llr_weighted(Y, n_bpsc, w48):
    with np.errstate(invalid="ignore", over="ignore"):
        return (llr(Y, n_bpsc) * _f32(w48)[..., None]).astype(np.float32)


def llr_bf16(values):
    """rule 15: the bf16 pattern of each float32 LLR"""
    return bf16_rne(values)


def planes(idx_row, n_bpsc, n_sym_out, max_sym):
    """the bit planes of one frame (include/wifirx.h, wifirx_out.hbits): [max_sym * 12] uint32, symbol q in the 2 n_bpsc
    words from q 2 n_bpsc on, word 2 b + h = bit b of bins 32 h .. 32 h + 31, bin 32 h + k in bit k; nothing behind the last
    symbol (left 0 here)"""
    out = [0] * (max_sym * 12)
    for q in range(n_sym_out):
        for b in range(n_bpsc):
            w = 0
            for c, i in enumerate(DATA_BINS):
                w |= ((int(idx_row[q][c]) >> b) & 1) << i
            out[q * 2 * n_bpsc + 2 * b] = w & 0xffffffff
            out[q * 2 * n_bpsc + 2 * b + 1] = w >> 32
    return np.array(out, dtype=np.uint32)
