"""NUMERICS.md rule 21 without a GPU: the prototype the built library hands out, tests/channelizer_ref.py against the direct
float64 definition, its invariance under cuts, and the bank in front of the oracle's receiver."""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

import channelizer_ref as zr
import convert_ref as cr
from wifirx import capi, txgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(M, s) for M in zr.CHANNELS for s in (0, 1)]


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("gen_channelizer_table", os.path.join(ROOT, "tools", "gen_channelizer_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("M", zr.CHANNELS)
def test_table_of_the_built_library(M):
    h = capi.channelizer_table(M)
    assert h.dtype == np.float32 and h.shape == (24 * M,) and np.isfinite(h).all()
    assert np.array_equal(h, h[::-1])                                  # exact symmetry
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= 2.0 ** -20
    dev, stop = gen().figures(h, M)
    print("M = %d: passband deviation %.3e, stopband %.2f dB" % (M, dev, stop))
    assert dev <= 3e-3
    assert stop <= -55.0


def test_committed_header_is_the_generator_s_and_the_library_s():
    g = gen()
    assert open(g.HEADER).read() == g.render()
    for M in zr.CHANNELS:
        assert np.array_equal(capi.channelizer_table(M), g.design(M))
        for got, want in zip(zr.branch_constants(M), g.branch_constants(M).T):
            assert np.array_equal(got, want)
        for got, want in zip(zr.twiddles(M), g.twiddles(M).T):
            assert np.array_equal(got, want)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.standard_normal(n), rng.standard_normal(n)], axis=1).astype(np.float32)


@pytest.mark.parametrize("M,s", CASES)
def test_restatement_against_the_direct_definition(M, s):
    """bound: every output is a sum of 24 rounded products per branch, 23 adds, and log2 M butterflies whose operands carry
    the branch constant's and a twiddle's roundings -- the rule counts 24 + 3 log2 M + 4 roundings of values bounded by
    sum |h| max |x| per part, two parts"""
    n_out = 300
    x = noise(n_out * M, 100 * M + s)
    h = zr.table(M)
    got = zr.analyse(x, M, s)
    want = zr.direct(cr.to_complex(x), M, s, h)
    assert got.shape == want.shape == (M, n_out)
    bound = (24 + 3 * math.log2(M) + 4) * 2.0 ** -24 * 2 * float(np.abs(h.astype(np.float64)).sum()) * float(np.abs(x).max())
    worst = float(np.abs(got.astype(np.complex128) - want).max())
    print("M = %d, s = %d: worst |restatement - definition| = %.3e, bound %.3e" % (M, s, worst, bound))
    assert worst <= bound


@pytest.mark.parametrize("M,s", CASES)
def test_restatement_is_invariant_under_cuts(M, s):
    n_out = 120
    x = noise(n_out * M, 7 * M + s)
    whole = zr.analyse(x, M, s, m0=5)
    for cut in (1, 23, 24, 25):
        a = zr.analyse(x[:cut * M], M, s, None, 5)
        hist = zr.next_history(x[:cut * M], None, M)
        b = zr.analyse(x[cut * M:], M, s, hist, 5 + cut)
        assert np.array_equal(np.concatenate([a, b], axis=1).view(np.uint32), whole.view(np.uint32)), cut


def test_m0_parity_is_all_that_matters_and_only_for_odd_stacking():
    x = noise(40 * 4, 3)
    assert np.array_equal(zr.analyse(x, 4, 1, m0=1), -zr.analyse(x, 4, 1, m0=0))
    assert np.array_equal(zr.analyse(x, 4, 1, m0=6), zr.analyse(x, 4, 1, m0=0))
    assert np.array_equal(zr.analyse(x, 4, 0, m0=1), zr.analyse(x, 4, 0, m0=0))


def test_integer_formats_are_widened_first():
    q = np.random.default_rng(4).integers(-128, 128, (64 * 2, 2)).astype(np.int8)
    got = zr.analyse_format(q, cr.SC8, 2.0 ** -7, 2, 1)
    assert np.array_equal(got, zr.analyse(cr.widen(q, 2.0 ** -7), 2, 1))


def test_synthesis_puts_each_stream_on_its_channel():
    """a tone at +fs/8 of channel k alone comes out of channel k, with unit gain, and at -55 dB or less of the others"""
    M, s, n = 4, 1, 1024
    tone = np.exp(2j * np.pi * 0.125 * np.arange(n))
    for k in range(M):
        streams = [tone if j == k else np.zeros(n) for j in range(M)]
        wide = zr.synthesise(streams, M, s).astype(np.complex64)
        y = zr.analyse(cr.pairs(wide), M, s)[:, 100:].astype(np.complex128)
        level = np.sqrt(np.mean(np.abs(y) ** 2, axis=1))
        assert abs(level[k] - 1.0) < 5e-3, (k, level)
        assert (np.delete(level, k) < 10 ** (-55 / 20)).all(), (k, level)


# ---- through the oracle ------------------------------------------------------------------------------------------------

def frame_stream(n_frames, seed, enc=7, plen=1528, lead=160, tail=240):
    psdu = txgen.make_psdus(n_frames, plen, seed=seed)
    tx = txgen.encode_psdus(psdu, enc)
    row = np.zeros((n_frames, lead + tx.samples.shape[1] + tail), np.complex128)
    row[:, lead:lead + tx.samples.shape[1]] = tx.samples
    return row.reshape(-1), tx.n_sym


def fcs_good(x, n_sym):
    from oracle import oracle as orc
    prm = orc.make_params(max_sym=n_sym)
    o = orc.demod_stream(np.asarray(x, dtype=np.complex64), prm, cap=64)
    orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
    return int(np.count_nonzero(o["frames"]["flags"] & capi.F_CRC_OK))


def test_bank_in_front_of_the_oracle_receiver():
    """M = 4, s = 1: 12 frames per channel of 64-QAM 3/4, 1528 bytes, noise of unit variance per channel bandwidth, the even
    channels at 28 dB and the odd ones 25 dB above them; each channel decodes at least what channel 0's stream decodes alone
    at 28 dB"""
    M, s, n_frames, snr_db = 4, 1, 12, 28.0
    rng = np.random.default_rng(21)
    streams, n_sym = [], 0
    for k in range(M):
        v, n_sym = frame_stream(n_frames, seed=50 + k)
        streams.append(v)
    n = len(streams[0])
    gains = [math.sqrt(10 ** ((snr_db + (25.0 if k & 1 else 0.0)) / 10)) for k in range(M)]
    alone = gains[0] * streams[0] + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * math.sqrt(0.5)
    baseline = fcs_good(alone, n_sym)
    wide = zr.synthesise(streams, M, s, gains)
    wide = wide + (rng.standard_normal(n * M) + 1j * rng.standard_normal(n * M)) * math.sqrt(0.5 * M)
    y = zr.analyse(cr.pairs(wide.astype(np.complex64)), M, s)
    good = [fcs_good(y[k], n_sym) for k in range(M)]
    print("FCS-good per channel %s, channel 0 alone %d of %d" % (good, baseline, n_frames))
    assert baseline >= n_frames // 2, "the operating point lost the link: the comparison would be of failures"
    assert all(g >= baseline for g in good), (good, baseline)
