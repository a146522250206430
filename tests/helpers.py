"""Shared helpers of the test-suite: synthetic slots with the reference's loop-back channel, the bit-plane layout of the
hard decisions, a fenced PSDU buffer on the device."""
import numpy as np

from soft_rows import FILL          # what a fenced buffer and its fences are filled with
from wifirx import txgen

DATA_BINS = np.array([i for i in range(6, 59) if i not in (11, 25, 32, 39, 53)])       # data carrier c -> FFT bin (shifted)
N_BPSC = np.array([1, 1, 2, 2, 4, 4, 6, 6])
FENCE = 4096                                 # bytes in front of and behind a fenced buffer


def make_slots(n_frames, encoding, psdu_len=294, snr_db=25.0, cfo_max=2e-5 * 5.89e9 / 20e6 * 2 * np.pi,
               lead=160, tail=320, seed=7, taps=None, jitter=0):
    """Returns (iq [n_frames*slot_len] complex64, slot_len, TxBatch)."""
    psdu = txgen.make_psdus(n_frames, psdu_len, seed=2025 + seed)
    tx = txgen.encode_psdus(psdu, encoding)
    n = tx.samples.shape[1]
    slot_len = ((lead + n + tail + 63) // 64) * 64
    rng = np.random.default_rng(seed)
    cfo = rng.uniform(-cfo_max, cfo_max, n_frames)
    iq = txgen.impair(tx.samples, snr_db, cfo=cfo, lead=lead, total=slot_len, seed=1234 + seed, taps=taps)
    return iq.reshape(-1), slot_len, tx


def planes_of(frames, idx, max_sym):
    """numpy statement of the layout in include/wifirx.h: word 2 b + h of symbol q = bit b of bins 32 h .. 32 h + 31"""
    n = len(frames)
    out = np.zeros((n, max_sym * 12), np.uint32)
    for f in range(n):
        nb = int(N_BPSC[frames["encoding"][f] & 7]) if frames["n_bpsc"][f] else 0
        for q in range(int(frames["n_sym_out"][f])):
            dec = idx[f, q].astype(np.uint32)
            for b in range(nb):
                bits = np.zeros(64, np.uint64)
                bits[DATA_BINS] = (dec >> b) & 1
                w = int((bits << np.arange(64, dtype=np.uint64)).sum())
                out[f, q * 2 * nb + 2 * b] = w & 0xffffffff
                out[f, q * 2 * nb + 2 * b + 1] = w >> 32
    return out


class Fenced:
    """a PSDU buffer of n rows, `off` bytes behind a 16-byte boundary, between two fences, all of it FILL"""

    def __init__(self, rx, n, stride, off=0):
        self.n, self.stride, self.at = n, stride, FENCE + off
        self.total = FENCE + 16 + n * stride + FENCE
        self.buf = rx.alloc(self.total).upload(np.full(self.total, FILL, np.uint8))
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + self.at

    def refill(self):
        self.buf.upload(np.full(self.total, FILL, np.uint8))

    def expected(self, rows):
        e = np.full(self.total, FILL, np.uint8)
        e[self.at:self.at + self.n * self.stride] = rows.reshape(-1)
        return e

    def download(self):
        return self.buf.download(np.uint8, self.total)

    def free(self):
        self.buf.free()
