"""NUMERICS.md rule 19 restated on the host: what wifirx_channel_fading (wr_channel.hip) computes, value for value -- the
Doppler fader in NumPy float32 between tests/resample_ref.py's rule 18 and the mixer, gain and noise of tests/channel_ref.py's
rule 17.

Row r, tap l, sinusoid k: the draw d = Philox4x32-10((8 l + k, r, 0, 1), fade_seed) (the line of sight of tap 0: index 128)
gives the arrival angle a = (float)(int32)d.x 2 pi / 2^32, the increment inc = llround((double)fd (double)cos(a) 2^64) and the
start phase phi = d.y : d.z.  On the 32-sample grid of t = time0 + n the gain is G_l(t) = 0.35355339 sum_k (cos, sin)(phi + inc t)
(ascending k, the parts summed apart), tap 0 with k_factor > 0 a_los e_los(t) + a_nlos G_0(t); between grid points it is
interpolated linearly, g = G(q) + w (G(q + 32) - G(q)), and s[n] = sum_l ch_mul(ch_mul(g_l(n), t_l), x[n - l])."""
import math

import numpy as np

import channel_ref
from channel_ref import F32, M64, PHASE_SCALE, philox4x32_10, angle
from oracle import oracle as orc
from wifirx import capi

SINES, STEP, LOS, MAX_TAPS = 8, 32, 128, 16
DOPPLER_MAX = 2.0 ** -10
AMP = F32(0.35355339)
U64 = np.uint64

# the end-to-end case of test_fading_ref.py (through the oracle) and test_gpu_fading.py (through the device chain): 48 frames of
# 64-QAM 2/3, 1528 bytes, a flat Rician channel at 30 dB without carrier offset; arms (name, doppler, equaliser)
E2E = dict(n=48, enc=6, plen=1528, lead=160, k_factor=10.0, snr_db=30.0, seed=30, fade_seed=4, psdu_seed=19)
ARMS = (("fd 1e-4, LS", 1e-4, capi.EQ_LS), ("fd 1e-4, STA", 1e-4, capi.EQ_STA), ("fd 0, LS", 0.0, capi.EQ_LS))


def oscillators(row, n_taps, fd, fade_seed):
    """(inc, phi): uint64 [..., 8 n_taps + 1] each, slot 8 l + k for sinusoid k of tap l, the last slot the line of sight.
    row and fd: scalars, or arrays of one shape (the leading axes of the result)"""
    row = np.asarray(row, dtype=np.uint32)
    idx = np.broadcast_to(np.concatenate([np.arange(SINES * n_taps), [LOS]]).astype(np.uint32), row.shape + (SINES * n_taps + 1,))
    d = philox4x32_10(idx, np.broadcast_to(row[..., None], idx.shape), np.zeros(idx.shape, np.uint32), np.ones(idx.shape, np.uint32),
                      fade_seed & 0xFFFFFFFF, (fade_seed >> 32) & 0xFFFFFFFF)
    _, cs = orc.sincos(d[0].view(np.int32).astype(F32) * PHASE_SCALE)
    v = np.asarray(fd, dtype=F32).astype(np.float64)[..., None] * cs.astype(np.float64) * 2.0 ** 64      # exact
    a = np.abs(v)
    k = np.where(a >= 2.0 ** 52, a, np.floor(a + 0.5))                   # llround: half away from zero
    inc = np.where(v < 0, -k, k).astype(np.int64).view(U64)              # |v| <= 2^54
    phi = (d[1].astype(U64) << U64(32)) | d[2].astype(U64)
    return inc, phi


def rice(k_factor):
    """(a_los, a_nlos) as float32, formed in double from the float32 value of k_factor; (0, 0): not applied"""
    K = float(F32(k_factor))
    if K <= 0.0:
        return F32(0), F32(0)
    return F32(math.sqrt(K / (K + 1.0))), F32(math.sqrt(1.0 / (K + 1.0)))


def osc(inc, phi, t):
    """(cos, sin) float32 of oscillators at the times t: uint64 arrays that broadcast"""
    with np.errstate(over="ignore"):
        P = np.asarray(phi, dtype=U64) + np.asarray(inc, dtype=U64) * np.asarray(t, dtype=U64)
    sn, cs = orc.sincos(angle(P))
    return cs, sn


def grid_gains(inc, phi, tq, n_taps, a_los=F32(0), a_nlos=F32(0)):
    """the gains at the grid times tq (uint64 [m]): (real, imaginary) float32 [..., m, n_taps]"""
    tq = np.asarray(tq, dtype=U64)
    inc, phi = inc[..., None], phi[..., None]                  # [..., slot, 1] against [m]
    Gr = np.empty(inc.shape[:-2] + (tq.size, n_taps), F32)
    Gi = np.empty_like(Gr)
    for l in range(n_taps):
        sr, si = osc(inc[..., SINES * l, :], phi[..., SINES * l, :], tq)
        for k in range(1, SINES):
            c, s = osc(inc[..., SINES * l + k, :], phi[..., SINES * l + k, :], tq)
            sr, si = sr + c, si + s
        gr, gi = AMP * sr, AMP * si
        if l == 0 and a_los != 0:
            c, s = osc(inc[..., -1, :], phi[..., -1, :], tq)
            gr, gi = a_los * c + a_nlos * gr, a_los * s + a_nlos * gi
        Gr[..., l], Gi[..., l] = gr, gi
    return Gr, Gi


def gains(t, inc, phi, n_taps, a_los=F32(0), a_nlos=F32(0)):
    """g_l at the stream times t (uint64 [n]): (real, imaginary) float32 [..., n, n_taps]"""
    t = np.asarray(t, dtype=U64)
    q = t & ~U64(STEP - 1)
    with np.errstate(over="ignore"):
        q1 = q + U64(STEP)
    tq = np.unique(np.concatenate([q, q1]))
    Gr, Gi = grid_gains(inc, phi, tq, n_taps, a_los, a_nlos)
    i0, i1 = np.searchsorted(tq, q), np.searchsorted(tq, q1)
    w = ((t & U64(STEP - 1)).astype(F32) * F32(1.0 / STEP))[:, None]
    G0r, G1r, G0i, G1i = (np.take(G, i, axis=-2) for G, i in ((Gr, i0), (Gr, i1), (Gi, i0), (Gi, i1)))
    return G0r + w * (G1r - G0r), G0i + w * (G1i - G0i)


def fading_row(x, taps, fd, k_factor=0.0, fade_seed=0, time0=0, inc=0, phase0=0, gain=1.0, noise_voltage=0.0, seed=0,
               sample0=0, row=0):
    """one row: x complex64 [n] (after the resampler), taps complex64 [L <= 16] -> complex64 [n]"""
    x = np.asarray(x, dtype=np.complex64)
    n = x.size
    t = np.asarray(taps, dtype=np.complex64).reshape(-1)
    assert 1 <= t.size <= MAX_TAPS and 0.0 <= float(F32(fd)) <= DOPPLER_MAX
    with np.errstate(over="ignore"):
        tt = U64(time0 & M64) + np.arange(n, dtype=U64)
    gr, gi = gains(tt, *oscillators(row, t.size, fd, fade_seed), t.size, *rice(k_factor))
    coef = [(gr[:, l] * F32(t[l].real) - gi[:, l] * F32(t[l].imag), gr[:, l] * F32(t[l].imag) + gi[:, l] * F32(t[l].real))
            for l in range(t.size)]
    return channel_ref.mix(*channel_ref.fir(x, coef), inc, phase0, gain, noise_voltage, seed, sample0, row)


def channel(x, row_off=None, taps=(1.0,), cfo=None, phase0=0, sro=None, drift0=0, gain=1.0, noise_voltage=0.0, seed=0,
            sample0=0, doppler=None, k_factor=0.0, fade_seed=0, time0=0):
    """WifiRx.channel(..., doppler=, k_factor=, fade_seed=, time0=) restated.  doppler: scalar or per row (taken as float32),
    None = rules 17 and 18 alone."""
    return channel_ref.channel(x, row_off, taps, cfo, phase0, gain, noise_voltage, seed, sample0, sro=sro, drift0=drift0,
                               doppler=doppler, k_factor=k_factor, fade_seed=fade_seed, time0=time0)
