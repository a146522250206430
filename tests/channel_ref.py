"""NUMERICS.md rule 17 restated on the host: what wifirx_channel (wr_channel.hip) computes, value for value.

Per row: the FIR in float32 (plain products and sums, ascending k from the k = 0 product), the mixer with the fixed-point
phase P = phase0 + inc n mod 2^64 and the oracle's sincos (rule 1), one float32 multiply by the gain per part, then -- when
noise_voltage != 0 -- Philox4x32-10 + Box-Muller noise on the counter ((sample0 + n) >> 1, row), key = seed.  The noiseless
path is bit-exact; the noise uses NumPy's float32 log / sqrt / sin / cos where the device has its own, so it agrees to ulps.

channel() composes rules 17 to 19: the row layout, the per-row arguments and the choice of the tap set are written here once,
the resampler's stages are resample_ref.py's and the fader's fading_ref.py's; fir() and mix() serve static and fading taps."""
import math

import numpy as np

from oracle import oracle as orc

F32 = np.float32
PHASE_SCALE = F32(2 * math.pi / 2 ** 32)
U01_SCALE = F32(2.3283064365386963e-10)
TWO_PI_F = F32(6.283185307179586)
M64 = (1 << 64) - 1


def phase_inc(cfo) -> int:
    """rad/sample (a float32 value) -> uint64 increment in 2^-64 turns: llround(cfo / (2 pi) * 2^64), the turns reduced to
    [-1/2, 1/2] first, +-1/2 turn = 2^63 (wifirx_api_channel.inc: channel_phase_inc)"""
    f = float(F32(cfo)) / 6.283185307179586
    f -= float(np.rint(f))
    v = f * 2.0 ** 64
    if v >= 2.0 ** 63 or v <= -2.0 ** 63:
        return 1 << 63
    a = abs(v)
    k = int(a) if a >= 2.0 ** 52 else math.floor(a + 0.5)      # llround: half away from zero (a + 0.5 is exact below 2^52)
    return (-k if v < 0 else k) & M64


def _mulhilo(a, b):
    p = a.astype(np.uint64) * np.uint64(b)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint32 each), key (k0, k1): four uint32 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32).copy() for c in (c0, c1, c2, c3))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    for _ in range(10):
        hi0, lo0 = _mulhilo(c0, 0xD2511F53)
        hi1, lo1 = _mulhilo(c2, 0xCD9E8D57)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = np.uint32((int(k0) + 0x9E3779B9) & 0xFFFFFFFF)
        k1 = np.uint32((int(k1) + 0xBB67AE85) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def u01(x):
    return (np.asarray(x, dtype=np.uint32).astype(F32) + F32(0.5)) * U01_SCALE


def noise(m, row, seed, noise_voltage):
    """complex64 noise of samples m (uint64 array, sample0 + n) of `row`"""
    m = np.asarray(m, dtype=np.uint64)
    j = m >> np.uint64(1)
    d = philox4x32_10((j & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.full(m.shape, row, np.uint32),
                      (j >> np.uint64(32)).astype(np.uint32), np.zeros(m.shape, np.uint32),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    odd = (m & np.uint64(1)) != 0
    ua, ub = np.where(odd, d[2], d[0]), np.where(odd, d[3], d[1])
    with np.errstate(divide="ignore"):
        r = np.sqrt(F32(-2.0) * np.log(u01(ua)))
    ang = TWO_PI_F * u01(ub)
    h = F32(0.70710678118654752) * F32(noise_voltage)
    return (h * r) * np.cos(ang), (h * r) * np.sin(ang)


def angle(P):
    """uint64 phases in 2^-64 turns -> the float32 angle the mixer forms"""
    return (P >> np.uint64(32)).astype(np.uint32).view(np.int32).astype(F32) * PHASE_SCALE


def fir(x, coef):
    """s[n] = sum_k c_k[n] x[n - k], x = 0 before the row: plain float32 products and sums per part, from the k = 0 product in
    ascending k.  x complex64 [n]; coef: per tap its (real, imaginary) parts, float32 scalars (a tap set) or arrays [n] (taps
    that vary per sample).  Returns the parts (real, imaginary) float32 [n]"""
    x = np.asarray(x, dtype=np.complex64)
    n = x.size
    xr, xi = x.real.astype(F32), x.imag.astype(F32)
    sr = np.zeros(n, F32)
    si = np.zeros(n, F32)
    for k, (ar, ai) in enumerate(coef):
        br = np.zeros(n, F32)
        bi = np.zeros(n, F32)
        if k < n:
            br[k:], bi[k:] = xr[:n - k], xi[:n - k]
        pr = ar * br - ai * bi
        pi = ar * bi + ai * br
        sr, si = (pr, pi) if k == 0 else (sr + pr, si + pi)
    return sr, si


def mix(sr, si, inc=0, phase0=0, gain=1.0, noise_voltage=0.0, seed=0, sample0=0, row=0):
    """rule 17 after the FIR: the mixer, the gain and the noise on the parts (sr, si) float32 [n] -> complex64 [n]"""
    idx = np.arange(sr.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        P = np.uint64(phase0 & M64) + np.uint64(inc & M64) * idx
    sn, cs = orc.sincos(angle(P))
    yr = sr * cs - si * sn
    yi = sr * sn + si * cs
    g = F32(gain)
    yr, yi = g * yr, g * yi
    if noise_voltage != 0.0:
        with np.errstate(over="ignore"):
            m = np.uint64(sample0 & M64) + idx
        wr_, wi_ = noise(m, row, seed, noise_voltage)
        yr, yi = yr + wr_, yi + wi_
    out = np.empty(sr.size, np.complex64)
    out.real, out.imag = yr, yi
    return out


def channel_row(x, taps, inc=0, phase0=0, gain=1.0, noise_voltage=0.0, seed=0, sample0=0, row=0):
    """one row: x complex64 [n], taps complex64 [L] -> complex64 [n]"""
    t = np.asarray(taps, dtype=np.complex64).reshape(-1)
    return mix(*fir(x, [(F32(c.real), F32(c.imag)) for c in t]), inc, phase0, gain, noise_voltage, seed, sample0, row)


def channel(x, row_off=None, taps=(1.0,), cfo=None, phase0=0, gain=1.0, noise_voltage=0.0, seed=0, sample0=0, *, sro=None,
            drift0=0, doppler=None, k_factor=0.0, fade_seed=0, time0=0):
    """WifiRx.channel restated, rules 17 to 19 composed: x [n_rows, row_len] (1-D = one row) or, with row_off, the 1-D buffer;
    taps 1-D or [n_tap_sets, L]; cfo, sro and doppler scalar or per row (taken as float32).  sro=None: no resampler
    (resample_ref.py), doppler=None: static taps (fading_ref.py).  Samples outside the rows are 0."""
    import fading_ref          # (both import this module)
    import resample_ref
    x = np.asarray(x, dtype=np.complex64)
    t = np.asarray(taps, dtype=np.complex64)
    t = t[None] if t.ndim == 1 else t
    if row_off is None:
        rows = x.reshape(1, -1) if x.ndim == 1 else x
        off = np.arange(rows.shape[0] + 1, dtype=np.uint64) * rows.shape[1]
        flat = rows.reshape(-1)
    else:
        off = np.asarray(row_off, dtype=np.uint64)
        flat = x
    n_rows = off.size - 1
    per_row = lambda v: None if v is None else np.broadcast_to(np.asarray(v, dtype=F32), (n_rows,))
    c, s, fd = per_row(0.0 if cfo is None else cfo), per_row(sro), per_row(doppler)
    assert s is None or (np.abs(s) <= resample_ref.SRO_MAX).all()
    out = np.zeros(flat.size, np.complex64)
    for r in range(n_rows):
        a, b = int(off[r]), int(off[r + 1])
        if b > a:
            u = flat[a:b] if s is None else resample_ref.resample_row(flat[a:b], resample_ref.drift_inc(s[r]), drift0)
            tail = (phase_inc(c[r]), phase0, gain, noise_voltage, seed, sample0, r)
            if fd is None:
                out[a:b] = channel_row(u, t[r % t.shape[0]], *tail)
            else:
                out[a:b] = fading_ref.fading_row(u, t[r % t.shape[0]], fd[r], k_factor, fade_seed, time0, *tail)
    return out.reshape(x.shape)
