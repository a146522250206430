"""NUMERICS.md rule 18 on the CPU: the resampler's table as the built library hands it out, tests/resample_ref.py against
float64 tones and against rule 17, and the sign of the locked sample clock through the oracle."""
import os
import zlib

import numpy as np
import pytest

import channel_ref
import resample_ref
from wifirx import capi, txgen

ONE = 1 << 40                       # one sample of drift


def cnoise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.5).astype(np.complex64)


# ---- 1. the table ----

def test_table_shape_and_unit_impulses():
    T = capi.resampler_table()
    assert T.shape == (129, 32) and T.dtype == np.float32
    for row, k in ((0, 15), (128, 16)):
        want = np.zeros(32, np.float32)
        want[k] = 1.0
        assert T[row].tobytes() == want.tobytes(), row       # exact, and +0 everywhere else
    assert np.isfinite(T).all()


def test_table_fidelity_over_the_occupied_band():
    """worst | sum_k c_k exp(j 2 pi f (k - 15)) - exp(j 2 pi f mu) | over |f| <= 26.5/64 and 1000 delays, the linear
    interpolation between rows included, in float64 on the float32 table: -60 dB, 25 dB under what 64-QAM needs"""
    T = capi.resampler_table().astype(np.float64)
    f = np.linspace(-26.5 / 64, 26.5 / 64, 531)
    E = np.exp(2j * np.pi * f[:, None] * (np.arange(32) - 15)[None, :])
    worst = 0.0
    for mu in (np.arange(1000) + 0.5) / 1000:
        p = int(mu * 128)
        frac = mu * 128 - p
        c = T[p] + frac * (T[p + 1] - T[p])
        worst = max(worst, float(np.abs(E @ c - np.exp(2j * np.pi * f * mu)).max()))
    print("worst response error %.3e" % worst)
    assert worst <= 1e-3


# ---- 2. the restatement against analytic tones ----

@pytest.mark.parametrize("sro,drift0,n", [(20e-6, int(0.3 * ONE), 4096), (-20e-6, int(0.3 * ONE), 4096),
                                          (2.0 ** -8, 0, 250), (-2.0 ** -8, int(0.99 * ONE), 250)])
def test_restatement_against_float64_tones(sro, drift0, n):
    """rows whose drift stays within one sample, so that outputs 16 .. n - 17 read inside the row"""
    dinc = resample_ref.drift_inc(sro)
    m = np.arange(n, dtype=np.float64)
    pos = m + (drift0 + dinc * np.arange(n, dtype=np.int64)).astype(np.float64) / ONE
    assert np.floor(pos[16]) - 15 >= 0 and np.floor(pos[n - 17]) + 16 <= n - 1
    worst = 0.0
    for k in range(-26, 27):
        x = np.exp(2j * np.pi * (k / 64) * m).astype(np.complex64)
        u = resample_ref.resample_row(x, dinc, drift0)
        want = np.exp(2j * np.pi * (k / 64) * pos)
        worst = max(worst, float(np.abs(u[16:n - 16] - want[16:n - 16]).max()))
    print("sro %g: worst distance from the tone %.3e" % (sro, worst))
    assert worst <= 1.1e-3


# ---- 3. no drift is rule 17; a row cut into two calls ----

def test_zero_sro_is_channel_ref_value_for_value():
    rng = np.random.default_rng(1)
    lens = [0, 1, 7, 31, 32, 33, 700]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(3)
    x = cnoise(rng, int(off[-1]) + 5)
    taps = ((rng.standard_normal((2, 8)) + 1j * rng.standard_normal((2, 8))) / 4).astype(np.complex64)
    cfo = rng.uniform(-0.05, 0.05, len(lens)).astype(np.float32)
    kw = dict(row_off=off, taps=taps, cfo=cfo, phase0=12345, gain=0.5, noise_voltage=0.2, seed=9, sample0=77)
    want = channel_ref.channel(x, **kw)
    got = resample_ref.channel(x, sro=np.zeros(len(lens), np.float32), drift0=0, **kw)
    assert got.tobytes() == want.tobytes()
    assert resample_ref.channel(x, sro=None, **kw).tobytes() == want.tobytes()


@pytest.mark.parametrize("sro", [20e-6, -20e-6, 2.0 ** -8, -2.0 ** -8])
@pytest.mark.parametrize("n_taps", [1, 8])
def test_cut_invariance(sro, n_taps):
    """the second call starts at sample k with drift0 and phase0 advanced: behind the 31 + n_taps samples that see the cut
    it equals the uncut row"""
    rng = np.random.default_rng(n_taps)
    n, k = 3000, 1234
    x = cnoise(rng, n)
    taps = ((rng.standard_normal(n_taps) + 1j * rng.standard_normal(n_taps)) / 4).astype(np.complex64)
    cfo = np.float32(0.021)
    d0 = int(0.4 * ONE)
    dinc, inc = resample_ref.drift_inc(sro), channel_ref.phase_inc(cfo)
    kw = dict(taps=taps, cfo=cfo, sro=sro, gain=1.5, noise_voltage=0.3, seed=5)
    one = resample_ref.channel(x, phase0=7, drift0=d0, **kw)
    # the second call's integer drift must stay within the halo: |D| < 16 samples here
    part = resample_ref.channel(x[k:], phase0=(7 + inc * k) & channel_ref.M64, drift0=d0 + dinc * k, sample0=k, **kw)
    halo = 31 + n_taps
    assert part[halo:].tobytes() == one[k + halo:].tobytes()
    assert part[:halo].tobytes() != one[k:k + halo].tobytes()


# ---- 4. the sign, through the oracle ----

def _fcs_good(frames, psdu, plen):
    ok = 0
    for f, row in zip(frames, psdu):
        if (f["flags"] & capi.F_COMPLETE) and f["psdu_len"] == plen:
            body = row[:plen].tobytes()
            ok += zlib.crc32(body[:-4]) == int.from_bytes(body[-4:], "little")
    return ok


def test_locked_clock_sign_through_the_oracle(orc):
    """48 frames of 64-QAM 3/4, 1528 bytes (57 symbols), +-20 ppm of 5.89 GHz at 20 MS/s, 32 dB, the LS equaliser: with the
    sample clock locked to the carrier (sro = -cfo bw / (2 pi fc)) the frames decode, with the carrier offset alone they do
    not -- the receiver compensates a drift that is not there"""
    n, enc, plen, lead = 48, 7, 1528, 160
    tx = txgen.encode_psdus(txgen.make_psdus(n, plen, seed=18), enc)
    assert tx.n_sym == 57
    flen = tx.samples.shape[1]
    slot = lead + flen + 79
    rows = np.zeros((n, slot), np.complex64)
    rows[:, lead:lead + flen] = tx.samples
    cfo = np.where(np.arange(n) % 2 == 0, 0.037, -0.037).astype(np.float32)
    locked = np.stack([resample_ref.resample_row(rows[r], resample_ref.drift_inc(resample_ref.locked_sro(cfo[r])))
                       for r in range(n)])
    prm = orc.make_params(max_sym=tx.n_sym, chan_est=capi.EQ_LS)
    threads = min(os.cpu_count() or 1, 8)
    good = {}
    for name, x in (("locked", locked), ("unlocked", rows)):
        iq = txgen.impair(x, 32.0, cfo=cfo.astype(np.float64), lead=0, total=slot, seed=32)
        o = orc.demod_batch(iq.reshape(-1), slot, prm, n_threads=threads)
        psdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=1536, n_threads=threads)
        good[name] = _fcs_good(o["frames"], psdu, plen)
    print("FCS-good of %d: %r" % (n, good))
    assert good["locked"] >= 45
    assert good["unlocked"] <= 3
