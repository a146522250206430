"""Host-built inputs of the stream-diversity tests, one table for tests/test_detect_multi_ref.py (CPU: the restatement of
tests/detect_multi_ref.py alone) and tests/test_gpu_stream_diversity.py (the device against it).

capture(A)       what wifirx_detect_multi is compared on bit for bit: N = 2 * 4096 + 3 * 64 + 37 samples per antenna (three
                 workgroups of the detection kernel, wave and tile boundaries, an odd tail); three frames, one across sample
                 4096, with a complex gain per antenna, in independent unit-variance noise, with exact-zero gaps.
rayleigh_scene   200 frame heads (preamble + SIGNAL + one symbol) at a mean SNR, flat Rayleigh fading independent per antenna
                 and frame, in unit-variance noise: the scene NUMERICS.md rule 24 quotes its detection counts for.
clean_stream     the ten-frame stream of tests/test_gpu_stream.py::build_stream (mixed rates and lengths, per-frame CFO,
                 roughly 40 k samples) without its noise; antenna() scales it and adds an antenna's own noise."""
import functools

import numpy as np

N_CAPTURE = 2 * 4096 + 3 * 64 + 37
ZERO_GAPS = ((0, 150), (2500, 3000), (8300, N_CAPTURE))


def _noise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _frame(plen=40, enc=0, seed=11):
    from wifirx import txgen
    return txgen.encode_psdus(txgen.make_psdus(1, plen, seed=seed), enc).samples[0]


@functools.lru_cache(maxsize=None)
def capture(n_ant, seed=41):
    """tuple of n_ant complex64 arrays of N_CAPTURE samples"""
    rng = np.random.default_rng(seed)
    f = _frame()
    assert f.size == 1601
    out = []
    for a in range(8):                                   # antenna a's samples do not depend on n_ant
        g = (rng.standard_normal(3) + 1j * rng.standard_normal(3)) * np.sqrt(0.5) * np.sqrt(10 ** (14 / 10))
        x = _noise(rng, N_CAPTURE).astype(np.complex128)
        for k, s in enumerate((400, 3600, 6600)):
            x[s:s + f.size] += g[k] * f * np.exp(1j * (0.01 * (k - 1)) * np.arange(f.size))
        for lo, hi in ZERO_GAPS:
            x[lo:hi] = 0
        out.append(x.astype(np.complex64))
    return tuple(out[:n_ant])


@functools.lru_cache(maxsize=None)
def rayleigh_scene(n_frames=200, snr_db=10.0, n_ant=4, seed=24, head=560, period=1024):
    """(tuple of n_ant streams, frame starts): frame k's head at starts[k], its complex gain drawn per antenna and frame"""
    rng = np.random.default_rng(seed)
    f = _frame(100, 2, 12)[:head]
    starts = 200 + period * np.arange(n_frames)
    n = int(starts[-1]) + period
    amp = np.sqrt(10 ** (snr_db / 10))
    xs = []
    for a in range(n_ant):
        x = _noise(rng, n).astype(np.complex128)
        h = (rng.standard_normal(n_frames) + 1j * rng.standard_normal(n_frames)) * np.sqrt(0.5)
        for k, s in enumerate(starts):
            x[s:s + head] += amp * h[k] * f
        xs.append(x.astype(np.complex64))
    return tuple(xs), starts


def frames_detected(triggers, starts, window=320):
    """how many frames have a trigger inside their preamble (the `window` samples from the frame's start on)"""
    t = np.sort(np.asarray(triggers, dtype=np.int64))
    k = np.searchsorted(t, starts)
    hit = (k < t.size) & (t[np.minimum(k, max(t.size - 1, 0))] < starts + window) if t.size else np.zeros(len(starts), bool)
    return int(np.count_nonzero(hit))


SPECS = [(0, 60), (2, 294), (4, 500), (7, 1000), (2, 294), (5, 120), (3, 294), (6, 64), (1, 200), (2, 294)]


@functools.lru_cache(maxsize=None)
def clean_stream(seed=3, snr_db=24.0):
    """(clean complex128 stream, PSDUs): frames with 100 front / 1000 tail padding in exact zeros, scaled to snr_db over unit noise"""
    from wifirx import txgen
    rng = np.random.default_rng(seed)
    parts, psdus = [], []
    for k, (enc, plen) in enumerate(SPECS):
        psdu = txgen.make_psdus(1, plen, seed=seed * 100 + k, seq0=k)
        tx = txgen.encode_psdus(psdu, enc, seeds=[(k % 127) + 1])
        n = tx.samples.shape[1]
        cfo = rng.uniform(-0.03, 0.03)
        sig = tx.samples[0] * np.exp(1j * cfo * np.arange(n)) * np.sqrt(10 ** (snr_db / 10))
        parts += [np.zeros(100, np.complex128), sig.astype(np.complex128), np.zeros(1000 if k != 4 else 200, np.complex128)]
        psdus.append(psdu[0])
    return np.concatenate(parts), psdus


def antenna(clean, gain=1.0, noise_seed=None):
    """one antenna's complex64 samples: gain * clean, plus unit-variance noise drawn from noise_seed (None: no noise)"""
    x = np.asarray(clean, dtype=np.complex128) * gain
    if noise_seed is not None:
        x = x + _noise(np.random.default_rng(noise_seed), x.size)
    return x.astype(np.complex64)
