"""NUMERICS.md rule 22 without a GPU: tests/combine_ref.py against the float64 definition, its invariance under cuts, where
each stream lands, the round trip through rule 21's analysis bank, and the pair of banks in front of the oracle's receiver."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import channelizer_ref as zr
import combine_ref as cb
import convert_ref as cr
import wideband_scene as ws
from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(M, s) for M in cb.CHANNELS for s in (0, 1)]
SCENE_SEED = 3


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("gen_channelizer_table", os.path.join(ROOT, "tools", "gen_channelizer_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def noise(rng, M, n):
    return (rng.standard_normal((M, n)) + 1j * rng.standard_normal((M, n))).astype(np.complex64)


@pytest.mark.parametrize("M,s", CASES)
def test_restatement_against_the_definition(M, s):
    """Roundings on the longest path of the rule, M = 8, stacking 1, each at most 2^-24 of a value that the terms' absolute
    sum bounds: the gain 1; the inverse DFT's three stages 1 + 1 + 4 (an add; the +j stage's add; the one stage with a
    rounded twiddle: the twiddle's own rounding, a product and a sum inside rule 17's product, and the add); the tap
    product 1; the 23 adds of the branch sum; the branch constant 3 (its own rounding, a product, a sum): 35, at most 40."""
    rng = np.random.default_rng(100 * M + s)
    n, m0 = 300, 7
    u, hist = noise(rng, M, n), noise(rng, M, 23)
    g = rng.uniform(-2, 2, M).astype(np.float32)
    h = zr.table(M)
    got = cb.combine(u, M, s, g, hist, m0)
    want = cb.direct(u, M, s, h, g, hist, m0)
    assert got.shape == want.shape == (n * M,) and got.dtype == np.complex64
    S = cb.term_sum(u, M, h, g, hist)
    ratio = np.abs(got.astype(np.complex128) - want) / (2.0 ** -24 * S)
    print("M = %d, s = %d: worst |restatement - definition| = %.2f x 2^-24 S[n], bound 40" % (M, s, ratio.max()))
    assert (ratio <= 40).all()
    # and from the start of a stream, without gains
    got0, want0 = cb.combine(u, M, s), cb.direct(u, M, s, h)
    assert (np.abs(got0.astype(np.complex128) - want0) <= 40 * 2.0 ** -24 * cb.term_sum(u, M, h)).all()


@pytest.mark.parametrize("M,s", CASES)
def test_a_cut_stream_is_the_uncut_stream(M, s):
    rng = np.random.default_rng(7 * M + s)
    n, m0 = 600, 5
    u = noise(rng, M, n)
    g = rng.uniform(-2, 2, M).astype(np.float32)
    whole = cb.combine(u, M, s, g, None, m0)
    for cut in (1, 22, 23, 24, 511, 512, 513):
        a = cb.combine(u[:, :cut], M, s, g, None, m0)
        hist = cb.next_history(u[:, :cut], None, M)
        b = cb.combine(u[:, cut:], M, s, g, hist, m0 + cut)
        assert np.array_equal(np.concatenate([a, b]).view(np.uint32), whole.view(np.uint32)), cut
        assert np.array_equal(cb.next_history(u[:, cut:], hist, M).view(np.uint32), cb.next_history(u, None, M).view(np.uint32)), cut


def test_m0_parity_is_all_that_matters_and_only_for_odd_stacking():
    u = noise(np.random.default_rng(3), 4, 40)
    assert np.array_equal(cb.combine(u, 4, 1, m0=1), -cb.combine(u, 4, 1, m0=0))
    assert np.array_equal(cb.combine(u, 4, 1, m0=6), cb.combine(u, 4, 1, m0=0))
    assert np.array_equal(cb.combine(u, 4, 0, m0=1), cb.combine(u, 4, 0, m0=0))


@pytest.mark.parametrize("M,s", CASES)
def test_each_stream_lands_on_its_own_channel(M, s):
    """a unit tone at f0 cycles per channel sample in channel k alone appears at f_k + f0 / M with the amplitude 1 to within
    the prototype's pass-band deviation, and at the M - 1 image positions f_k + f0 / M + i / M below its stop-band figure
    plus 0.5 dB; the figures are gen_channelizer_table.py --check's (2.0e-3; -58.4 .. -58.9 dB).  The deviation is reached
    at the band's edge, |f0| = 26.5 / 64, by the definition itself, so the float32 restatement is given its forward bound on
    top of it: 40 x 2^-24 x the largest branch's sum |M h| for a unit tone (the first test; 3e-6, 0.15 % of the deviation)."""
    h = capi.channelizer_table(M)
    dev, stop_db = gen().figures(h, M)
    f32 = 40 * 2.0 ** -24 * float(np.abs(h.astype(np.float64) * M).reshape(-1, M).sum(axis=0).max())
    assert dev <= 2.05e-3 and -59.0 <= stop_db <= -58.3
    win, lead = 1024, 48                                      # the window holds whole cycles of every tone below
    n = lead + win
    t = np.arange(lead * M, n * M)
    worst_amp, worst_img = 0.0, 0.0
    for k in range(M):
        for f0 in (-26.5 / 64, -13 / 64, 0.0, 5 / 64, 26 / 64, 26.5 / 64):
            u = np.zeros((M, n), np.complex64)
            u[k] = np.exp(2j * np.pi * f0 * np.arange(n))
            x = cb.combine(u, M, s)[lead * M:].astype(np.complex128)
            at = zr.centre(k, M, s) + f0 / M
            level = [abs(np.mean(x * np.exp(-2j * np.pi * (at + i / M) * t))) for i in range(M)]
            worst_amp, worst_img = max(worst_amp, abs(level[0] - 1.0)), max(worst_img, max(level[1:]))
            assert abs(level[0] - 1.0) <= dev + f32, (k, f0, level)
            assert 20 * np.log10(max(level[1:])) <= stop_db + 0.5, (k, f0, level)
    print("M = %d, s = %d: |amplitude - 1| <= %.2e (deviation %.2e), images <= %.2f dB (stop band %.2f dB)"
          % (M, s, worst_amp, dev, 20 * np.log10(worst_img), stop_db))


@functools.lru_cache(maxsize=None)
def synthesis(M, s):
    """the noiseless scene through rule 22 in float32: complex64 [n M]"""
    x = cb.combine(ws.streams(M, SCENE_SEED).astype(np.complex64), M, s)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("M,s", CASES)
def test_round_trip_through_the_analysis_bank(M, s):
    """independent code on the way back: channelizer_ref.analyse gives every stream back delayed by 23 samples; what is left
    is the frames' own spectral skirts outside the banks' pass band: measured 1.2e-2 .. 1.7e-2 of a stream's rms over the
    whole stream (1.3e-2 inside the frames, the rest ringing in the gaps).  The bound is 2e-2; a swapped channel, a
    conjugated twiddle or a wrong block sign gives O(1)."""
    u = ws.streams(M, SCENE_SEED)
    y = zr.analyse(cr.pairs(synthesis(M, s)), M, s).astype(np.complex128)
    assert y.shape == u.shape
    for k in range(M):
        err = np.sqrt(np.sum(np.abs(y[k, 23:] - u[k, :-23]) ** 2) / np.sum(np.abs(u[k, :-23]) ** 2))
        print("M = %d, s = %d, channel %d: rms error %.3e of the frames' rms" % (M, s, k, err))
        assert err <= 2e-2, (k, err)


@pytest.mark.parametrize("M,s", CASES)
def test_both_banks_in_front_of_the_oracle_receiver(M, s):
    """synthesis, noise of unit variance per channel bandwidth, sc16 at 12 dB back-off, analysis, the oracle's receiver: every
    transmitted PSDU is delivered with a good FCS"""
    from oracle import oracle as orc
    chans, n = ws.layout(M, SCENE_SEED)
    wide = (synthesis(M, s).astype(np.complex128) + ws.wide_noise(M, n, SCENE_SEED)).astype(np.complex64)
    scale_q = cr.full_scale(wide, 12.0, cr.SC16)
    q, _ = cr.quantise(cr.pairs(wide), scale_q, cr.SC16)
    rows = zr.analyse_format(q, cr.SC16, np.float32(1.0 / float(scale_q)), M, s)
    for k in range(M):
        prm = orc.make_params(bandwidth=20e6, frequency=5.21e9 + zr.centre(k, M, s) * M * 20e6, max_sym=511)
        o = orc.demod_stream(np.asarray(rows[k]), prm, cap=64)
        psdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
        assert len(o["frames"]) == len(chans[k]), (k, len(o["frames"]))
        assert ((o["frames"]["flags"] & capi.F_CRC_OK) != 0).all(), k
        for i, frame in enumerate(chans[k]):
            sent = frame[2]
            assert int(o["frames"]["psdu_len"][i]) == len(sent) and np.array_equal(psdu[i, :len(sent)], sent), (k, i)
