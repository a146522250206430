"""CPU reference of the hard-decision decode_mac (`wifirx_decode_batch`; NUMERICS.md rule 14a), NumPy int64, vectorised
over frames.

Test infrastructure only: the package never imports it, and it is written from the rule (the comments of
csrc/wr_decode.hip / csrc/wr_decode.h), not from the oracle -- tests/test_hard_rows.py holds the two against each other.

* which frames (`frame_steps`): WIFIRX_F_COMPLETE set, psdu_len <= psdu_stride, psdu_len <= 1528, and the symbols of a
  PSDU of psdu_len bytes at the record's rate, n_sym, <= min(max_sym, 511); every other record is left as it is;
* input: `idx` [n][max_sym][48] -- bit k of a byte is coded bit k of the carrier, bits at or above n_bpsc are ignored;
  coded bits are placed by the de-puncturing and the de-interleaver (`soft_viterbi_ref.llr_map`);
* metrics: Hamming branch metrics (a punctured position costs nothing), integer path metrics that are NEVER normalised
  (int64: nothing a kernel does to keep its metrics small can be mirrored here by accident); start: state 0 at 0, the
  others unreachable;
* add-compare-select: c0 = pm[p0] + bm0, c1 = pm[p1] + bm1, candidate 1 only if c1 < c0, the survivor bit is c1 < c0;
* end: smallest metric, lowest state on ties; trace-back over n_sym * n_dbps steps; descramble from the first seven
  bits; CRC-32, WIFIRX_F_CRC_OK needs psdu_len >= 4.

Next to the decode it measures what the byte metrics of decode_q_kernel rest on (`Margins`), and per frame how often
the tie rules decided.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from soft_viterbi_ref import (F_COMPLETE, F_CRC_OK, F_DECODED, MAX_PSDU, MAX_SYM, N_BPSC, N_DBPS, finish, llr_map,
                              n_sym_of)

UNREACHABLE = 1 << 40          # start metric of the states != 0: beyond any path of 511 * 216 steps
SETTLED = 6                    # from this many steps on every state has a survivor that started in state 0
WINDOW = 48                    # decode_q_kernel: the common minimum leaves the metrics every so many steps


def _taps(r):
    """expected coded pair of register r (bit k = the input k steps ago): generators 133 and 171 octal, 133 first"""
    a = (r ^ (r >> 2) ^ (r >> 3) ^ (r >> 5) ^ (r >> 6)) & 1
    b = (r ^ (r >> 1) ^ (r >> 2) ^ (r >> 3) ^ (r >> 6)) & 1
    return 2 * a + b


# state s = the six newest inputs, the newest in bit 0; its predecessors are s >> 1 (older bit 0) and s >> 1 | 32
_S = np.arange(64)
_P0, _P1 = _S >> 1, (_S >> 1) | 32
_E0 = _taps((_P0 << 1) | (_S & 1))
_E1 = _taps((_P1 << 1) | (_S & 1))


@dataclass
class Margins:
    """largest values seen, over frames and steps; the first two from step SETTLED on"""
    spread: int = 0            # max - min of a frame's 64 metrics
    cand_diff: int = 0         # |c1 - c0| of a state
    growth: int = 0            # growth of a frame's minimum over WINDOW consecutive steps

    def merge(self, o: "Margins"):
        self.spread, self.cand_diff, self.growth = max(self.spread, o.spread), max(self.cand_diff, o.cand_diff), max(self.growth, o.growth)


def decodable(frames: np.ndarray, max_sym: int, psdu_stride: int) -> np.ndarray:
    enc = frames["encoding"].astype(np.int64) & 7
    ln = frames["psdu_len"].astype(np.int64)
    nd = np.array(N_DBPS)[enc]
    n_sym = (16 + 8 * ln + 6 + nd - 1) // nd
    return ((frames["flags"] & F_COMPLETE) != 0) & (ln <= psdu_stride) & (ln <= MAX_PSDU) & (n_sym <= min(max_sym, MAX_SYM))


def coded_bits(idx: np.ndarray, enc: int, psdu_len: int) -> np.ndarray:
    """idx [F][>= n_sym][48] -> the de-punctured coded stream [F][2 n_steps]: 0, 1, or 2 where the transmitter dropped the bit"""
    n_sym, nb = n_sym_of(enc, psdu_len), N_BPSC[enc]
    m = llr_map(enc)
    bits = (idx[:, :n_sym, :, None] >> np.arange(nb, dtype=np.uint8)) & 1          # [F][sym][carrier][bit]
    c = bits.reshape(idx.shape[0], n_sym, 48 * nb)[:, :, np.where(m < 0, 0, m)]
    c[:, :, m < 0] = 2
    return c.reshape(idx.shape[0], -1)


def viterbi_hard(coded: np.ndarray):
    """coded uint8 [F][2 n] in {0, 1, 2}.  Returns (decoded bits uint8 [F][n], Margins, ties met on the surviving path
    int64 [F], final minimum held by more than one state bool [F])."""
    F, n2 = coded.shape
    n = n2 // 2
    miss = np.stack([(coded != 2) & (coded != 0), (coded != 2) & (coded != 1)], axis=2).astype(np.int64)      # cost of expecting 0 / 1
    bm = miss[:, 0::2, [0, 0, 1, 1]] + miss[:, 1::2, [0, 1, 0, 1]]                                           # [F][n][2 a + b]
    pm = np.full((F, 64), UNREACHABLE, np.int64)
    pm[:, 0] = 0
    surv = np.empty((n, F, 8), np.uint8)
    tied = np.empty((n, F, 8), np.uint8)
    mins = np.zeros((n + 1, F), np.int64)
    mg = Margins()
    for t in range(n):
        b = bm[:, t]
        c0 = pm[:, _P0] + b[:, _E0]
        c1 = pm[:, _P1] + b[:, _E1]
        take = c1 < c0
        if t >= SETTLED:
            mg.cand_diff = max(mg.cand_diff, int(np.abs(c1 - c0).max()))
        pm = np.where(take, c1, c0)
        surv[t] = np.packbits(take, axis=1, bitorder="little")
        tied[t] = np.packbits(c1 == c0, axis=1, bitorder="little")
        mins[t + 1] = pm.min(axis=1)
        if t + 1 >= SETTLED:
            mg.spread = max(mg.spread, int((pm.max(axis=1) - mins[t + 1]).max()))
    if n >= WINDOW:
        mg.growth = int((mins[WINDOW:] - mins[:-WINDOW]).max())
    s = np.argmin(pm, axis=1)                                 # the first minimum: lowest state on ties
    final_tied = (pm == mins[n][:, None]).sum(axis=1) > 1
    out = np.empty((F, n), np.uint8)
    n_ties = np.zeros(F, np.int64)
    rows = np.arange(F)
    for t in range(n - 1, -1, -1):
        out[:, t] = s & 1
        n_ties += (tied[t][rows, s >> 3] >> (s & 7)) & 1
        h = (surv[t][rows, s >> 3] >> (s & 7)) & 1
        s = (s >> 1) | (h.astype(np.int64) << 5)
    assert (s == 0).all()                                     # every surviving path starts in state 0
    return out, mg, n_ties, final_tied


def decode_batch(frames: np.ndarray, idx: np.ndarray, max_sym: int, psdu_stride: int = 2048, chunk: int = 512):
    """The contract over a batch.  frames: FRAME_DTYPE [n]; idx: uint8 [n][max_sym][48].
    Returns (frames with F_DECODED / F_CRC_OK updated, psdu uint8 [n][psdu_stride], zero where nothing was decoded, and
    dict(margins, ties [n], final_tied [n], steps [n]) -- the last three 0 / False for frames left alone)."""
    frames = frames.copy()
    n = frames.shape[0]
    psdu = np.zeros((n, psdu_stride), np.uint8)
    info = dict(margins=Margins(), ties=np.zeros(n, np.int64), final_tied=np.zeros(n, bool), steps=np.zeros(n, np.int64))
    sel = np.nonzero(decodable(frames, max_sym, psdu_stride))[0]
    key = (frames["encoding"][sel].astype(np.int64) & 7) * 65536 + frames["psdu_len"][sel]
    for k in np.unique(key):
        grp = sel[key == k]
        enc, ln = int(k) >> 16, int(k) & 0xFFFF
        for c0 in range(0, grp.size, chunk):
            g = grp[c0:c0 + chunk]
            dec, mg, ties, final_tied = viterbi_hard(coded_bits(idx[g], enc, ln))
            by, ok = finish(dec, ln)
            psdu[g, :ln] = by
            fl = frames["flags"][g] | F_DECODED
            frames["flags"][g] = np.where(ok, fl | F_CRC_OK, fl & ~np.uint32(F_CRC_OK))
            info["margins"].merge(mg)
            info["ties"][g], info["final_tied"][g], info["steps"][g] = ties, final_tied, dec.shape[1]
    return frames, psdu, info
