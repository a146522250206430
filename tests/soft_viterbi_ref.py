"""CPU reference of the soft-decision decode_mac (NUMERICS.md rule 14), NumPy float32, vectorised over frames.

Test infrastructure only: the package never imports it.  It restates the contract that
`wifirx_decode_batch_soft` (csrc/wr_decode_soft.hip) meets bit for bit:

* which frames: the ones the hard decoder takes (complete, PSDU fits the row, n_sym <= max_sym) that also carry
  WIFIRX_F_LLR; every other record is left as it is;
* coded bit -> LLR: de-puncture, then the de-interleaver of the hard path; inside a frame's row the LLR of data
  symbol q, carrier k, bit b sits at (q*48 + k)*n_bpsc + b, positive = bit 1;
* cost of a coded bit with LLR L: a non-finite L and a punctured position count as 0; cost0 = max(L, 0),
  cost1 = max(-L, 0); branch metric = cost_A + cost_B (first coded bit, generator 133, on the left), float32;
* add-compare-select: m0 = pm[p0] + bm0, m1 = pm[p1] + bm1, m1 taken only if m1 < m0 (survivor bit = m1 < m0);
* start: state 0 at 0, the other states at +inf; before every step t > 0 with t % NORM_STEPS == 0 the minimum of
  the 64 metrics is subtracted from all of them;
* end: smallest metric, lowest state on ties; trace back over the hard path's trellis length, descramble, CRC-32;
* overflow: plain IEEE float32, nothing clamped.  Metrics may reach +inf; when all 64 are +inf at a normalisation
  (LLR magnitudes around 1e37 and above) inf - inf makes all 64 NaN, no comparison is true from then on, and the
  survivor bits and the end state are 0.  A frame's metrics are NaN in none or in all 64 states (asserted below at
  every normalisation and at the end): that is what makes min / argmin here and fminf / the `<` scan of the kernel
  interchangeable.
"""
from __future__ import annotations

import zlib

import numpy as np

NORM_STEPS = 24            # WR_SOFT_NORM_STEPS of csrc/wr_decode_soft.hip
MAX_SYM = 511              # WIFIRX_MAX_SYM
MAX_PSDU = 1528            # WIFIRX_MAX_PSDU
F_COMPLETE, F_LLR, F_DECODED, F_CRC_OK = 0x08, 0x10, 0x20, 0x40
N_BPSC = (1, 1, 2, 2, 4, 4, 6, 6)
N_DBPS = (24, 36, 48, 72, 96, 144, 192, 216)
PUNCT = (0, 2, 0, 2, 0, 2, 1, 2)           # 0: 1/2, 1: 2/3, 2: 3/4


def _parity(v):
    return bin(v).count("1") & 1


# trellis: state s = (older bits << 1 | newest bit) & 63; predecessors p0 = s >> 1 and p1 = p0 | 32
_S = np.arange(64)
_P0 = _S >> 1
_P1 = _P0 | 32
_AB0 = np.array([2 * _parity(((p << 1) | (s & 1)) & 0o155) + _parity(((p << 1) | (s & 1)) & 0o117) for s, p in zip(_S, _P0)])
_AB1 = np.array([2 * _parity(((p << 1) | (s & 1)) & 0o155) + _parity(((p << 1) | (s & 1)) & 0o117) for s, p in zip(_S, _P1)])


def llr_map(enc: int) -> np.ndarray:
    """[2 * n_dbps]: where the de-punctured coded bit ci of one OFDM symbol sits among the symbol's 48 * n_bpsc LLRs
    (carrier * n_bpsc + bit), -1 where the transmitter dropped it."""
    n_bpsc, n_dbps, punct = N_BPSC[enc], N_DBPS[enc], PUNCT[enc]
    n_cbps = 48 * n_bpsc
    s = max(n_bpsc // 2, 1)
    out = np.empty(2 * n_dbps, dtype=np.int64)
    for ci in range(2 * n_dbps):
        if punct == 1:
            r = ci & 3
            if r == 3:
                out[ci] = -1
                continue
            k = (ci >> 2) * 3 + r
        elif punct == 2:
            g, r = divmod(ci, 6)
            if r in (3, 4):
                out[ci] = -1
                continue
            k = g * 4 + (r if r < 3 else 3)
        else:
            k = ci
        i = (n_cbps // 16) * (k % 16) + k // 16
        out[ci] = s * (i // s) + (i + n_cbps - (16 * i) // n_cbps) % s
    return out


def n_sym_of(enc: int, psdu_len: int) -> int:
    return (16 + 8 * psdu_len + 6 + N_DBPS[enc] - 1) // N_DBPS[enc]


def decodable(frames: np.ndarray, max_sym: int, psdu_stride: int) -> np.ndarray:
    """The frames the soft decoder takes: the hard decoder's rule (decode_maxsteps) and WIFIRX_F_LLR."""
    enc = frames["encoding"].astype(np.int64) & 7
    ln = frames["psdu_len"].astype(np.int64)
    nd = np.array(N_DBPS)[enc]
    n_sym = (16 + 8 * ln + 6 + nd - 1) // nd
    fl = frames["flags"]
    return (((fl & F_COMPLETE) != 0) & ((fl & F_LLR) != 0) & (ln <= psdu_stride) & (ln <= MAX_PSDU) &
            (n_sym <= MAX_SYM) & (n_sym <= max_sym))


def _scrambler_table(n_bits: int) -> np.ndarray:
    """[128][n_bits]: the feedback bit at every position i >= 7 of a descrambler started from state s (the first seven
    decoded bits, oldest in bit 6); the sequence does not depend on the data."""
    tab = np.zeros((128, n_bits), dtype=np.uint8)
    for s0 in range(128):
        st = s0
        for i in range(7, n_bits):
            fb = ((st >> 6) ^ (st >> 3)) & 1
            tab[s0, i] = fb
            st = ((st << 1) & 0x7E) | fb
    return tab


_SCR = None


def _none_or_all_nan(pm: np.ndarray) -> np.ndarray:
    """[F] bool: the frames whose metrics are NaN; a frame with some but not all 64 NaN is outside the contract"""
    n_nan = np.isnan(pm).sum(axis=1)
    assert np.all((n_nan == 0) | (n_nan == 64)), "a frame's 64 metrics are partly NaN"
    return n_nan == 64


def viterbi_soft(coded: np.ndarray, nan_frames: list | None = None) -> np.ndarray:
    """coded: float32 [F][2 n] -- the sanitised LLR of every de-punctured coded bit (0 = no information).
    Returns the decoded bits uint8 [F][n].  nan_frames (a list): gets one bool array [F], the frames that ended in the
    all-NaN regime."""
    coded = np.asarray(coded, dtype=np.float32)
    F, n2 = coded.shape
    n = n2 // 2
    zero = np.float32(0)
    pm = np.full((F, 64), np.inf, dtype=np.float32)
    pm[:, 0] = 0
    surv = np.empty((n, F, 8), dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n):
            if t and t % NORM_STEPS == 0:
                pm = pm - pm.min(axis=1, keepdims=True)          # inf - inf = NaN: the overflow regime
                _none_or_all_nan(pm)
            la, lb = coded[:, 2 * t], coded[:, 2 * t + 1]
            ca = np.stack([np.maximum(la, zero), np.maximum(-la, zero)], axis=1)      # cost of expecting 0 / 1
            cb = np.stack([np.maximum(lb, zero), np.maximum(-lb, zero)], axis=1)
            bm = np.stack([ca[:, 0] + cb[:, 0], ca[:, 0] + cb[:, 1], ca[:, 1] + cb[:, 0], ca[:, 1] + cb[:, 1]], axis=1)
            m0 = pm[:, _P0] + bm[:, _AB0]
            m1 = pm[:, _P1] + bm[:, _AB1]
            take = m1 < m0
            pm = np.where(take, m1, m0)
            surv[t] = np.packbits(take, axis=1, bitorder="little")
    is_nan = _none_or_all_nan(pm)
    if nan_frames is not None:
        nan_frames.append(is_nan)
    s = np.where(is_nan, 0, np.argmin(pm, axis=1))          # first minimum = lowest state; no `<` is true among NaNs
    out = np.empty((F, n), dtype=np.uint8)
    rows = np.arange(F)
    for t in range(n - 1, -1, -1):
        out[:, t] = s & 1
        h = (surv[t][rows, s >> 3] >> (s & 7)) & 1
        s = (s >> 1) | (h.astype(np.int64) << 5)
    return out


def coded_llrs(llr_rows: np.ndarray, enc: int, psdu_len: int) -> np.ndarray:
    """LLR rows [F][>= n_sym * 48 * n_bpsc] -> the sanitised de-punctured coded stream [F][2 n_data], float32."""
    n_sym = n_sym_of(enc, psdu_len)
    n_cbps = 48 * N_BPSC[enc]
    m = llr_map(enc)
    pos = (np.arange(n_sym)[:, None] * n_cbps + np.where(m < 0, 0, m)[None, :]).reshape(-1)
    c = np.asarray(llr_rows, dtype=np.float32)[:, pos]
    c = np.where(np.isfinite(c), c, np.float32(0)).astype(np.float32)
    c[:, np.tile(m < 0, n_sym)] = 0
    return c


def finish(dec: np.ndarray, psdu_len: int):
    """decoded bits [F][n] -> (PSDU bytes [F][psdu_len], CRC ok [F])"""
    global _SCR
    n_bits = 16 + 8 * psdu_len
    if _SCR is None or _SCR.shape[1] < n_bits:
        _SCR = _scrambler_table(max(n_bits, 16 + 8 * MAX_PSDU))
    s0 = np.zeros(dec.shape[0], dtype=np.int64)
    for i in range(7):
        s0 |= dec[:, i].astype(np.int64) << (6 - i)
    bits = dec[:, 16:n_bits] ^ _SCR[s0, 16:n_bits]
    by = np.packbits(bits, axis=1, bitorder="little")
    ok = np.array([psdu_len >= 4 and zlib.crc32(r.tobytes()) == 558161692 for r in by], dtype=bool)
    return by, ok


def decode_batch(frames: np.ndarray, llr: np.ndarray, max_sym: int, psdu_stride: int = 2048, chunk: int = 1024,
                 llr_bits: int = 6, nan_out: np.ndarray | None = None):
    """The contract over a batch.  frames: FRAME_DTYPE [n]; llr: float32 [n][max_sym*48*llr_bits].
    Returns (frames with F_DECODED / F_CRC_OK updated, psdu uint8 [n][psdu_stride]).  llr_bits: frames of a rate with more
    bits per carrier have no LLRs in the row and are left alone.  nan_out (bool [n]): set where a frame ended all-NaN."""
    frames = frames.copy()
    n = frames.shape[0]
    psdu = np.zeros((n, psdu_stride), dtype=np.uint8)
    fits = np.array(N_BPSC)[frames["encoding"].astype(np.int64) & 7] <= llr_bits
    sel = np.nonzero(decodable(frames, max_sym, psdu_stride) & fits)[0]
    if sel.size == 0:
        return frames, psdu
    key = (frames["encoding"][sel].astype(np.int64) & 7) * 65536 + frames["psdu_len"][sel]
    for k in np.unique(key):
        grp = sel[key == k]
        enc, ln = int(k) >> 16, int(k) & 0xFFFF
        for c0 in range(0, grp.size, chunk):
            g = grp[c0:c0 + chunk]
            nf = []
            dec = viterbi_soft(coded_llrs(llr[g], enc, ln), nf)
            if nan_out is not None:
                nan_out[g] = nf[0]
            by, ok = finish(dec, ln)
            psdu[g, :ln] = by
            fl = frames["flags"][g] | F_DECODED
            frames["flags"][g] = np.where(ok, fl | F_CRC_OK, fl & ~np.uint32(F_CRC_OK))
    return frames, psdu


def pm1_llrs(frames: np.ndarray, idx: np.ndarray, max_sym: int, llr_bits: int) -> np.ndarray:
    """LLR rows of +-1 built from the hard decisions (idx [n][max_sym][48]): +1 where the decided bit is 1.  Fed to the
    soft decoder they must reproduce the hard decoder exactly (every metric is then a small integer)."""
    n = frames.shape[0]
    out = np.zeros((n, max_sym * 48 * llr_bits), dtype=np.float32)
    for enc_nb in sorted(set(N_BPSC)):
        rows = np.nonzero((np.array(N_BPSC)[frames["encoding"].astype(np.int64) & 7] == enc_nb) &
                          ((frames["flags"] & F_LLR) != 0))[0]
        if rows.size == 0 or enc_nb > llr_bits:
            continue
        b = (idx[rows].astype(np.uint32)[..., None] >> np.arange(enc_nb, dtype=np.uint32)) & 1      # [r][sym][48][nb]
        out[rows, :max_sym * 48 * enc_nb] = np.where(b == 1, 1.0, -1.0).reshape(rows.size, -1)
    return out
