"""The scene of tests/test_gpu_spectrum_scan.py: an 80 MS/s capture, built like tune_ref.three_channel_scene, that holds
QPSK 1/2 frames of 100 bytes at -25 and +25 MHz only, 20 dB above the noise in their band, with noise-only gaps of more than
four survey rows between the frames; the centre candidate is idle.  sc16."""
import functools
import math

import numpy as np

import arb_ref as ar
import convert_ref as cr
import spectrum_ref as sr

RATE, CANDIDATES, BUSY = 80e6, (-25e6, 0.0, 25e6), (-25e6, 25e6)
ENC, PLEN, SNR_DB, N_FRAMES = 2, 100, 20.0, 3
LEAD, TAIL = 160, 1500                                        # channel samples around a frame: a gap of 1660 is 6.5 rows
N_FFT, HOP, AVG, WIDTH = 256, 256, 4, 20e6                    # a row is 1024 capture samples = 256 channel samples
FMT = cr.SC16


@functools.lru_cache(maxsize=None)
def scene():
    """(sc16 items [n, 2], scale, {offset: PSDUs}): the outer channels' frames start 100 channel samples apart, so 1560 channel
    samples (6 rows) between frames hold noise in every band"""
    from wifirx import txgen
    wide, psdus = 0.0, {}
    for k, off in enumerate(BUSY):
        p = txgen.make_psdus(N_FRAMES, PLEN, seed=36 + k)
        tx = txgen.encode_psdus(p, ENC)
        row = np.zeros((N_FRAMES, LEAD + tx.samples.shape[1] + TAIL), np.complex128)
        row[:, LEAD:LEAD + tx.samples.shape[1]] = tx.samples
        v = np.roll(row.reshape(-1), 100 * k) * math.sqrt(10 ** (SNR_DB / 10))
        up = ar.stream(v, 1, 4, n_out=4 * len(v)).astype(np.complex128)
        j = np.arange(len(up))
        wide = wide + up * np.exp(2j * np.pi * ((j * round(off / RATE * 16)) % 16) / 16.0)          # +-5/16 turn per sample
        psdus[off] = p
    rng = np.random.default_rng(37)
    wide = wide + (rng.standard_normal(len(wide)) + 1j * rng.standard_normal(len(wide))) * math.sqrt(2.0)
    wide = wide.astype(np.complex64)
    scale_q = cr.full_scale(wide, 12.0, FMT)
    q, _ = cr.quantise(cr.pairs(wide), scale_q, FMT)
    q.setflags(write=False)
    return q, np.float32(1.0 / float(scale_q)), psdus


def bands():
    return [sr.band(off, WIDTH, RATE, N_FFT) for off in CANDIDATES]


@functools.lru_cache(maxsize=None)
def survey():
    """the restatement's (rows [n_rows, 256], band rows [n_rows, 3]) of the scene: Blackman-Harris, SUM, norm 1"""
    q, scale, _ = scene()
    rows = sr.spectrum_format(q, FMT, scale, N_FFT, HOP, AVG, sr.BLACKMAN_HARRIS, sr.SUM)
    band_rows = sr.bands(rows, bands())
    rows.setflags(write=False)
    band_rows.setflags(write=False)
    return rows, band_rows
