"""NUMERICS.md rule 16 restated on the host: the transmitter's float32 arithmetic, value for value what wifirx_tx_batch
computes.  The bits (data_idx, signal_idx) come from txgen.encode_psdus; the frequency-domain values are the float32 roundings
of txgen's float64 ones; the IFFT is conj(FFT(conj(ifftshift(X)))) with the FFT of rule 4 (the oracle's fft64 in SPEC
mode), then one float32 multiply by (float)(1/sqrt(52)) and the roll-off 0.5f a + 0.5f b."""
import math

import numpy as np

from oracle import oracle as orc
from wifirx import txgen

SCALE = np.float32(1.0 / math.sqrt(52.0))
HALF = np.float32(0.5)


def freq_symbols(tx: txgen.TxBatch) -> np.ndarray:
    """[F, 5 + n_sym, 64] complex64, shifted order: sync words, SIGNAL, data symbols with pilots."""
    F, n_sym = tx.psdu.shape[0], tx.n_sym
    n_bpsc = txgen.RATE_TABLE[tx.encoding][0]
    X = np.zeros((F, 5 + n_sym, 64), dtype=np.complex64)
    X[:, 0:4, :] = txgen.sync_words().astype(np.complex64)[None]
    X[:, 4, txgen.DATA_BINS] = (2.0 * tx.signal_idx.astype(np.float64) - 1.0).astype(np.complex64)
    pts = txgen.constellation_points(n_bpsc).astype(np.complex64)
    X[:, 5:, txgen.DATA_BINS] = pts[tx.data_idx]
    p = txgen.polarity_sequence()[np.arange(n_sym + 1) % 127].astype(np.complex64)
    for b, sgn in zip(txgen.PILOT_BINS, (1, 1, 1, -1)):
        X[:, 4:, b] = p * np.complex64(sgn)
    return X


def ifft_spec(X: np.ndarray) -> np.ndarray:
    """[..., 64] shifted spectrum (complex64) -> time samples [..., 64] (complex64), rule 16."""
    shp = X.shape
    inp = np.conj(np.fft.ifftshift(X.reshape(-1, 64), axes=-1)).astype(np.complex64)
    y = np.fft.ifftshift(np.conj(orc.fft64(inp)), axes=-1)        # fft64 returns the shifted order
    re = y.real.astype(np.float32) * SCALE
    im = y.imag.astype(np.float32) * SCALE
    return (re + 1j * im.astype(np.float64)).astype(np.complex64).reshape(shp)


def roll_off(x: np.ndarray) -> np.ndarray:
    """[F, n_tot, 64] time symbols -> [F, n_tot * 80 + 1] frames: CP 16, first CP sample 0.5f own + 0.5f the previous
    symbol's continuation, one trailing half sample."""
    F, n_tot, _ = x.shape
    re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
    out = []
    for part in (re, im):
        sym = np.concatenate([part[:, :, 48:], part], axis=2)       # [F, n_tot, 80]
        first = HALF * part[:, :, 48]
        first[:, 1:] = first[:, 1:] + HALF * part[:, :-1, 0]
        sym[:, :, 0] = first
        o = np.empty((F, n_tot * 80 + 1), dtype=np.float32)
        o[:, :n_tot * 80] = sym.reshape(F, -1)
        o[:, n_tot * 80] = HALF * part[:, -1, 0]
        out.append(o)
    res = np.empty(out[0].shape, dtype=np.complex64)
    res.real, res.imag = out
    return res


def encode(psdu: np.ndarray, encoding: int, seeds=None) -> np.ndarray:
    """[F, L] uint8 -> [F, (5 + n_sym) * 80 + 1] complex64, what wifirx_tx_batch writes for these frames."""
    tx = txgen.encode_psdus(psdu, encoding, seeds)
    return roll_off(ifft_spec(freq_symbols(tx)))


def encode_list(psdus, encoding, seeds=None):
    """PSDUs of mixed lengths (list of bytes) -> list of frames, each built by encode() with its own seed."""
    n = len(psdus)
    seeds = (np.arange(n) % 127) + 1 if seeds is None else np.broadcast_to(np.asarray(seeds), (n,))
    return [encode(np.frombuffer(bytes(p), dtype=np.uint8)[None], encoding, [int(seeds[i])])[0] for i, p in enumerate(psdus)]
