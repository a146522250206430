"""The stream of the sample-format tests (tests/test_convert_ref.py on the oracle, tests/test_gpu_stream_formats.py on the
device): three frames of 60-byte PSDUs at three rates, 30 dB over unit-variance noise, +-20 ppm of carrier offset, foo.packet_pad2's
zeros around them (100 in front, 1000 behind; gnu_radio/IRS_user.py:193) and 4000 samples of noise alone in front -- about
11 k samples, more than the 8192 of the batch size the device test stages them with.  Built once per process."""
import functools

import numpy as np

import convert_ref as cr
from wifirx import txgen

BACKOFF_DB = 12.0
PLEN = 60
CFO_MAX = 2e-5 * 5.89e9 / 20e6 * 2 * np.pi      # 20 ppm at 5.89 GHz and 20 MS/s, rad/sample
# 64-QAM 3/4 closes each stream; the issue lets the sc8 arm fall back to 16-QAM 1/2 should 8 bits at 12 dB not carry it --
# they do (test_convert_ref.test_stream_condition checks it through the oracle), so both arms use the same rates
RATES = {cr.SC16: (0, 4, 7), cr.SC8: (0, 4, 7)}


@functools.lru_cache(maxsize=None)
def stream(fmt, seed=11):
    """(float32 stream x, its PSDUs, integers q [n, 2], scale_q, widened stream w, scale_w) for a format: q = rule-20
    quantisation of x with full scale BACKOFF_DB above the RMS of x's frames, w = q widened by 1 / scale_q rounded to float32"""
    rng = np.random.default_rng(seed)
    parts, psdus, busy = [np.zeros(4000, np.complex64)], [], [np.zeros(4000, bool)]
    for k, enc in enumerate(RATES[fmt]):
        psdu = txgen.make_psdus(1, PLEN, seed=seed * 100 + k, seq0=k)
        tx = txgen.encode_psdus(psdu, enc, seeds=[k + 1])
        n = tx.samples.shape[1]
        cfo = rng.uniform(-CFO_MAX, CFO_MAX)
        sig = tx.samples[0] * np.exp(1j * cfo * np.arange(n)) * np.sqrt(10 ** (30.0 / 10))
        parts += [np.zeros(100, np.complex64), sig.astype(np.complex64), np.zeros(1000, np.complex64)]
        busy += [np.zeros(100, bool), np.ones(n, bool), np.zeros(1000, bool)]
        psdus.append(psdu[0])
    x = np.concatenate(parts)
    x = (x + (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * np.sqrt(0.5)).astype(np.complex64)
    scale_q = cr.full_scale(x[np.concatenate(busy)], BACKOFF_DB, fmt)      # the level of the frames, as a receiver's gain is set
    q, _ = cr.quantise(cr.pairs(x), scale_q, fmt)
    scale_w = np.float32(1.0 / float(scale_q))
    w = cr.to_complex(cr.widen(q, scale_w))
    for a in (x, q, w):
        a.setflags(write=False)
    return x, tuple(psdus), q, scale_q, w, scale_w


@functools.lru_cache(maxsize=None)
def oracle_result(fmt, soft=False):
    """the oracle's stream result on the widened samples: (dict of demod_stream, PSDUs); soft: records as a handle with
    llr_bits = 6 writes them (WIFIRX_P_STREAM_SOFT), PSDUs by the soft reference decoder"""
    from oracle import oracle as orc
    w = stream(fmt)[4]
    if soft:
        import soft_viterbi_ref as sref
        o = orc.demod_stream(w, orc.make_params(max_sym=511, llr_bits=6), want_eq=True, cap=64)
        fr, psdu = sref.decode_batch(o["frames"], o["llr"], 511, psdu_stride=2048)
        o = dict(o, frames=fr)
        return o, psdu
    prm = orc.make_params(max_sym=511)
    o = orc.demod_stream(w, prm, want_eq=True, cap=64)
    psdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
    return o, psdu
