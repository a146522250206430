"""NUMERICS.md rule 19 on the CPU: tests/fading_ref.py reduces to rules 17 and 18 without Doppler, its interpolated gains stay
within the derived bound of float64 sinusoids, the draws have the mean power, the Clarke correlation and the Rician mean they
should, a stream may be cut anywhere, and through the oracle a Doppler of 1e-4 cycles per sample breaks the LS equaliser's
link and not the STA equaliser's."""
import math
import os
import zlib

import numpy as np
import pytest
from scipy.special import j0

import channel_ref
import fading_ref
import resample_ref
from wifirx import capi, txgen

U64 = np.uint64


def cnoise(rng, n):
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.5).astype(np.complex64)


# ---- 1. no Doppler is rules 17 and 18 ----

@pytest.mark.parametrize("sro", [None, 20e-6])
def test_no_doppler_is_resample_ref_bytewise(sro):
    rng = np.random.default_rng(2)
    lens = [0, 1, 7, 33, 700]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(3)
    x = cnoise(rng, int(off[-1]) + 5)
    taps = ((rng.standard_normal((2, 8)) + 1j * rng.standard_normal((2, 8))) / 4).astype(np.complex64)
    kw = dict(row_off=off, taps=taps, cfo=rng.uniform(-0.05, 0.05, len(lens)).astype(np.float32), phase0=12345, sro=sro,
              drift0=0 if sro is None else 12345678901, gain=0.5, noise_voltage=0.2, seed=9, sample0=77)
    want = resample_ref.channel(x, **kw)
    got = fading_ref.channel(x, doppler=None, k_factor=10.0, fade_seed=4, time0=99, **kw)
    assert got.tobytes() == want.tobytes()
    assert fading_ref.channel(x, doppler=0.0, **kw).tobytes() != want.tobytes()      # fd = 0 is a static draw, not "off"


# ---- 2. the interpolation against float64 sinusoids ----

def _exact_gains(t, inc, phi, n_taps):
    """float64 sum of the 8 sinusoids per tap from the same (inc, phi): complex128 [n, n_taps]"""
    with np.errstate(over="ignore"):
        P = phi[None, :] + inc[None, :] * np.asarray(t, dtype=U64)[:, None]
    e = np.exp(2j * np.pi * (P.astype(np.float64) / 2.0 ** 64))
    return e[:, :8 * n_taps].reshape(len(t), n_taps, 8).sum(axis=2) / math.sqrt(8.0), e[:, -1]


@pytest.mark.parametrize("fd", [1e-4, 2.0 ** -10])
@pytest.mark.parametrize("time0", [0, (1 << 40) + 12345])
def test_interpolation_within_the_derived_bound(fd, time0):
    """one sinusoid of amplitude 1/sqrt(8) deviates from its chord by at most theta^2 / 8 of its amplitude, theta = 2 pi fd 32
    the angle it turns between two grid points; 8 of them by sqrt(8) theta^2 / 8; float32 adds 2e-6"""
    theta = 2 * math.pi * float(np.float32(fd)) * 32
    bound = math.sqrt(8.0) * theta ** 2 / 8 + 2e-6
    t = U64(time0) + np.arange(4096, dtype=U64)
    worst = 0.0
    for row in range(4):
        inc, phi = fading_ref.oscillators(row, 8, fd, 77)
        gr, gi = fading_ref.gains(t, inc, phi, 8)
        exact, _ = _exact_gains(t, inc, phi, 8)
        worst = max(worst, float(np.abs((gr.astype(np.float64) + 1j * gi.astype(np.float64)) - exact).max()))
    print("fd %g time0 %d: worst distance %.3e, bound %.3e" % (fd, time0, worst, bound))
    assert worst <= bound


# ---- 3. the statistics of the draws ----

ROWS = np.arange(4096)
FD = np.full(ROWS.size, 1e-4, np.float32)


def test_mean_power_is_one():
    """E|g|^2 = 1 and Var|g|^2 = 7/8 for the sum of 8 unit phasors over sqrt(8)"""
    inc, phi = fading_ref.oscillators(ROWS, 8, FD, 2024)
    gr, gi = fading_ref.gains([1000003], inc, phi, 8)
    p = (gr.astype(np.float64) ** 2 + gi.astype(np.float64) ** 2).reshape(-1)
    se = math.sqrt(0.875 / p.size)
    print("mean |g|^2 = %.5f over %d draws, standard error %.5f" % (p.mean(), p.size, se))
    assert p.size == 4096 * 8 and abs(p.mean() - 1.0) <= 4 * se


def test_correlation_is_clarkes():
    """E[g(t) conj(g(t + tau))] = J0(2 pi fd tau) for arrival angles uniform on the circle"""
    inc, phi = fading_ref.oscillators(ROWS, 8, FD, 2025)
    t0 = 64 * 12345
    taus = [512, 2048, 5120]                       # grid times: the interpolation stays out of it
    gr, gi = fading_ref.gains([t0] + [t0 + tau for tau in taus], inc, phi, 8)
    g = gr.astype(np.float64) + 1j * gi.astype(np.float64)              # [rows, 4, taps]
    n = g.shape[0] * g.shape[2]
    for i, tau in enumerate(taus):
        c = (g[:, 0, :] * np.conj(g[:, 1 + i, :])).mean()
        want = j0(2 * math.pi * float(FD[0]) * tau)
        print("tau %d: correlation %.4f%+.4fj, J0 = %.4f, allowed %.4f" % (tau, c.real, c.imag, want, 4 / math.sqrt(n)))
        assert abs(c - want) <= 4 / math.sqrt(n)


def test_rician_mean():
    """g_0 conj(e_los) = a_los + a_nlos G_0 conj(e_los): mean a_los, variance a_nlos^2 = 1 / (K + 1)"""
    K = 10.0
    a_los, a_nlos = fading_ref.rice(K)
    assert a_los == np.float32(math.sqrt(10 / 11)) and a_nlos == np.float32(math.sqrt(1 / 11))
    inc, phi = fading_ref.oscillators(ROWS, 1, FD, 2026)
    t = np.array([32 * 777], U64)                  # a grid time: g_0 there is the rule's own sum
    gr, gi = fading_ref.gains(t, inc, phi, 1, a_los, a_nlos)
    c, s = fading_ref.osc(inc[:, -1], phi[:, -1], t[0])
    m = ((gr[:, 0, 0].astype(np.float64) + 1j * gi[:, 0, 0]) * (c.astype(np.float64) - 1j * s)).mean()
    se = math.sqrt((1.0 / (K + 1.0)) / ROWS.size)
    print("mean of g_0 conj(e_los) = %.4f%+.4fj, a_los = %.4f, standard error %.4f" % (m.real, m.imag, a_los, se))
    assert abs(m - float(a_los)) <= 4 * se
    # without a line of sight the scalings are not applied at all
    assert fading_ref.rice(0.0) == (0, 0)


# ---- 4. a stream cut into two calls ----

@pytest.mark.parametrize("n_taps", [1, 8, 16])
@pytest.mark.parametrize("time0", [0, (1 << 40) + 12345])
def test_cut_invariance(n_taps, time0):
    rng = np.random.default_rng(n_taps)
    n, k = 6000, 2345
    x = cnoise(rng, n)
    taps = ((rng.standard_normal(n_taps) + 1j * rng.standard_normal(n_taps)) / 4).astype(np.complex64)
    cfo = np.float32(0.021)
    inc = channel_ref.phase_inc(cfo)
    kw = dict(taps=taps, cfo=cfo, gain=1.5, noise_voltage=0.3, seed=5, doppler=3e-4, k_factor=10.0, fade_seed=6)
    one = fading_ref.channel(x, phase0=7, time0=time0, **kw)
    part = fading_ref.channel(x[k:], phase0=(7 + inc * k) & channel_ref.M64, sample0=k, time0=time0 + k, **kw)
    halo = n_taps - 1
    assert part[halo:].tobytes() == one[k + halo:].tobytes()
    if halo:
        assert part[:halo].tobytes() != one[k:k + halo].tobytes()
    # the grid lies on the stream time: another time0 gives other samples
    assert fading_ref.channel(x[k:], phase0=(7 + inc * k) & channel_ref.M64, sample0=k, time0=time0 + k + 1,
                              **kw)[halo:].tobytes() != one[k + halo:].tobytes()


# ---- 5. end to end through the oracle ----

def _fcs_good(frames, psdu, plen):
    ok = 0
    for f, row in zip(frames, psdu):
        if (f["flags"] & capi.F_COMPLETE) and f["psdu_len"] == plen:
            body = row[:plen].tobytes()
            ok += zlib.crc32(body[:-4]) == int.from_bytes(body[-4:], "little")
    return ok


E2E, ARMS = fading_ref.E2E, fading_ref.ARMS


def test_doppler_breaks_ls_and_not_sta_through_the_oracle(orc):
    """48 frames of 64-QAM 2/3, 1528 bytes (64 symbols), a flat Rician channel with K = 10 at 30 dB without carrier offset:
    at fd = 1e-4 cycles per sample (1 kHz at 10 MS/s) the channel turns away from the LS estimate of the preamble within the
    frame and the STA equaliser follows it; a static draw (fd = 0) costs LS nothing.  A float64 model of the same fader gave
    5-7, 46-47 and 48 frames; the rule's own draws with fade_seed 4 give 5, 48 and 48 (13, 48, 48 to 5, 46, 48 over six seeds)."""
    n, enc, plen, lead = E2E["n"], E2E["enc"], E2E["plen"], E2E["lead"]
    tx = txgen.encode_psdus(txgen.make_psdus(n, plen, seed=E2E["psdu_seed"]), enc)
    assert tx.n_sym == 64
    flen = tx.samples.shape[1]
    slot = lead + flen + 79
    rows = np.zeros((n, slot), np.complex64)
    rows[:, lead:lead + flen] = tx.samples
    threads = min(os.cpu_count() or 1, 8)
    good, made = {}, {}
    for name, fd, eq in ARMS:
        if fd not in made:
            made[fd] = fading_ref.channel(rows, gain=math.sqrt(10 ** (E2E["snr_db"] / 10)), noise_voltage=1.0, seed=E2E["seed"],
                                          doppler=fd, k_factor=E2E["k_factor"], fade_seed=E2E["fade_seed"])
        prm = orc.make_params(max_sym=tx.n_sym, chan_est=eq)
        o = orc.demod_batch(made[fd].reshape(-1), slot, prm, n_threads=threads)
        psdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=1536, n_threads=threads)
        good[name] = _fcs_good(o["frames"], psdu, plen)
    print("FCS-good of %d: %r" % (n, good))
    assert good["fd 1e-4, LS"] <= 15
    assert good["fd 1e-4, STA"] >= 40
    assert good["fd 0, LS"] >= 40
