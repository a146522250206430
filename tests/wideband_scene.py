"""The scene of tests/test_gpu_wideband.py, stated once for the synthesis bank's tests: two frames per channel, one encoding
per channel, PSDU lengths and gaps that fit no grid, 30 dB over noise of unit variance per channel bandwidth."""
import functools

import numpy as np

from wifirx import txgen

SNR_DB = 30.0
CFO_MAX = 2e-5 * 5.2e9 / 20e6 * 2 * np.pi          # 20 ppm, rad per channel sample
ENCODINGS = (0, 3, 5, 7, 2, 4, 6, 1)
PSDU_LENS = ((61, 135), (77, 203), (93, 58), (149, 111), (64, 65), (66, 67), (68, 69), (70, 71))


@functools.lru_cache(maxsize=None)
def layout(M, seed):
    """(frames per channel, n): a frame is (offset in channel samples, encoding, PSDU with FCS, scrambler seed, CFO in rad
    per sample, samples of the frame); n is the common length of the channel streams"""
    rng = np.random.default_rng(seed)
    chans, n = [], 0
    for k in range(M):
        pos = 1237 + 211 * k + int(rng.integers(0, 97))
        mine = []
        for j, plen in enumerate(PSDU_LENS[k]):
            psdu = txgen.make_psdus(1, plen, seed=seed * 100 + 10 * k + j, seq0=j)
            n_samp = txgen.encode_psdus(psdu, ENCODINGS[k], seeds=[1 + 2 * k + j]).samples.shape[1]
            mine.append((pos, ENCODINGS[k], psdu[0], 1 + 2 * k + j, float(rng.uniform(-CFO_MAX, CFO_MAX)), n_samp))
            pos += n_samp + 901 + 173 * j + 59 * k + int(rng.integers(0, 131))
        chans.append(tuple(mine))
        n = max(n, pos)
    return tuple(chans), n + 333


@functools.lru_cache(maxsize=None)
def streams(M, seed, snr_db=SNR_DB):
    """the channel streams made on the host in float64, noiseless, at `snr_db` over unit noise: complex128 [M, n], read-only"""
    chans, n = layout(M, seed)
    u = np.zeros((M, n), np.complex128)
    for k, frames in enumerate(chans):
        for pos, enc, psdu, sseed, cfo, n_samp in frames:
            tx = txgen.encode_psdus(psdu[None, :], enc, seeds=[sseed])
            u[k, pos:pos + n_samp] = tx.samples[0] * np.exp(1j * cfo * np.arange(n_samp)) * np.sqrt(10 ** (snr_db / 10))
    u.setflags(write=False)
    return u


def wide_noise(M, n, seed):
    """unit variance per channel bandwidth: variance M over the M times wider band, complex128 [n M]"""
    rng = np.random.default_rng(seed + 1000)
    return (rng.standard_normal(n * M) + 1j * rng.standard_normal(n * M)) * np.sqrt(0.5 * M)
