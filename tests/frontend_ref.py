"""The receive front end restated on the host: NUMERICS.md rule 32 (DC removal and blind IQ correction of a stream) and the
receiver impairments of wifirx_rx_impair, value for value.

Written from the rule's text.  NumPy float32 for what the rule computes in float32, Python integers for the statistics (a
block's sums are taken with int64 NumPy sums first: 4096 terms of at most 2^49 cannot leave int64) and Python floats, which
are IEEE doubles with correctly rounded sqrt and divide, for the image coefficient.  Imports nothing of the product or the
oracle; `fma32` is tests/detect_ref.py's exact float32 fused multiply-add."""
import math

import numpy as np

from detect_ref import fma32

BLOCK = 4096
LOG2_BLOCK = 12
RING = 64
CLAMP = 2 ** 24 - 1
FE_DC, FE_IQ = 1, 2
FC32, SC16, SC8 = 0, 1, 2

f32 = np.float32

STATE_DTYPE = np.dtype([("n", "<u8"), ("part", "<i8", (5,)), ("ring", "<i8", (RING, 5)), ("d0", "<i8", (2,)), ("w0", "<f4", (2,))])


def widen(x, fmt=FC32, scale=1.0):
    """the float pairs rule 20 produces, float32 [n, 2]: complex64 samples as they are, int16 / int8 [n, 2] times `scale`"""
    if fmt == FC32:
        return np.ascontiguousarray(np.asarray(x, dtype=np.complex64).reshape(-1)).view(np.float32).reshape(-1, 2).copy()
    return np.asarray(x).reshape(-1, 2).astype(np.float32) * f32(scale)


def fix(c, frac_bits):
    """one component in Q-F: t = x 2^F in float32, NaN -> 0, else rint clamped to +-(2^24 - 1); int64"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(c, dtype=np.float32) * f32(2.0 ** frac_bits)
        r = np.clip(np.rint(t), -float(CLAMP), float(CLAMP))
    return np.where(np.isnan(t), 0.0, r).astype(np.int64)


def sums5(u, v):
    """the five sums of a run of samples, as Python integers"""
    return [int(u.sum()), int(v.sum()), int((u * u + v * v).sum()), int((u * u - v * v).sum()), int((2 * u * v).sum())]


def window_shift(shift, b):
    """log2 W of block b >= 1: min(shift, ilog2(b))"""
    return min(shift, b.bit_length() - 1)


def image_coefficient(q):
    """w from the iq window's five means (Mi, Mq, Qp, Qr, Qi): fp64, one rounding per written operation"""
    mi, mq, qp, qr, qi = q
    P = float(qp - (mi * mi + mq * mq))
    Cr = float(qr - (mi * mi - mq * mq))
    Ci = float(qi - 2 * mi * mq)
    disc = P * P - (Cr * Cr + Ci * Ci)
    if not (P > 0) or disc < 0:
        return f32(0), f32(0)
    den = P + math.sqrt(disc)
    return f32(Cr / den), f32(Ci / den)


def apply(x, d, w):
    """y = x - d, z = y - w conj(y) on float32 pairs [n, 2]; every operation one float32 rounding"""
    with np.errstate(over="ignore", invalid="ignore"):
        yr, yi = x[:, 0] - d[0], x[:, 1] - d[1]
        cr = (yr * w[0]) + (yi * w[1])
        ci = (yr * w[1]) - (yi * w[0])
        return np.stack([yr - cr, yi - ci], axis=1).astype(np.float32)


class Frontend:
    """One stream's front end: process() takes the next samples, however the stream is cut."""

    def __init__(self, flags=FE_DC, frac_bits=12, dc_shift=2, iq_shift=4, state=None):
        self.flags, self.frac_bits, self.dc_shift, self.iq_shift = flags, frac_bits, dc_shift, iq_shift
        self.n = 0
        self.part = [0] * 5
        self.ring = [[0] * 5 for _ in range(RING)]
        self.d0 = [0, 0]
        self.w0 = [f32(0), f32(0)]
        if state is not None:
            st = np.asarray(state, dtype=STATE_DTYPE).reshape(())
            self.n = int(st["n"])
            self.part = [int(v) for v in st["part"]]
            self.ring = [[int(v) for v in row] for row in st["ring"]]
            self.d0 = [int(v) for v in st["d0"]]
            self.w0 = [f32(v) for v in st["w0"]]

    def state(self):
        st = np.zeros((), STATE_DTYPE)
        st["n"], st["part"], st["ring"], st["d0"], st["w0"] = self.n, self.part, self.ring, self.d0, self.w0
        return st

    def _offset(self, m):
        return [f32(float(m[0]) * 2.0 ** -self.frac_bits), f32(float(m[1]) * 2.0 ** -self.frac_bits)]

    def _window(self, b, shift, n_comp):
        s = window_shift(shift, b)
        return [sum(self.ring[bb % RING][i] for bb in range(b - (1 << s), b)) >> s for i in range(n_comp)]

    def correction(self, b):
        """(d, w) of block b, the ring holding the blocks in front of it"""
        if b == 0:
            d, w = self._offset(self.d0), list(self.w0)
        else:
            d = self._offset(self._window(b, self.dc_shift, 2))
            w = list(image_coefficient(self._window(b, self.iq_shift, 5)))
        if not self.flags & FE_DC:
            d = [f32(0), f32(0)]
        if not self.flags & FE_IQ:
            w = [f32(0), f32(0)]
        return d, w

    def estimate(self):
        """what the block of the next sample is corrected with: (dc, w) as complex64"""
        d, w = self.correction(self.n >> LOG2_BLOCK)
        return np.complex64(complex(d[0], d[1])), np.complex64(complex(w[0], w[1]))

    def process(self, x, fmt=FC32, scale=1.0):
        """the next samples of the stream -> complex64 [n]"""
        x = widen(x, fmt, scale)
        out = np.empty_like(x)
        pos = 0
        while pos < len(x):
            b, off = self.n >> LOG2_BLOCK, self.n & (BLOCK - 1)
            seg = x[pos:pos + BLOCK - off]
            d, w = self.correction(b)
            out[pos:pos + len(seg)] = apply(seg, d, w)
            s = sums5(fix(seg[:, 0], self.frac_bits), fix(seg[:, 1], self.frac_bits))        # always on the raw x
            self.part = [a + c for a, c in zip(self.part, s)]
            self.n += len(seg)
            if self.n & (BLOCK - 1) == 0:
                self.ring[b % RING] = [a >> LOG2_BLOCK for a in self.part]
                self.part = [0] * 5
            pos += len(seg)
        return out.view(np.complex64).reshape(-1)


def frontend(x, fmt=FC32, scale=1.0, **kw):
    """one call over a whole stream: (complex64 [n], state record)"""
    fe = Frontend(**kw)
    z = fe.process(x, fmt, scale)
    return z, fe.state()


def imbalance(gain_db=0.0, phase_deg=0.0):
    """(mu, nu) of a Q branch with gain g = 10^(gain_db / 20) and phase error phi: mu = (1 + g e^{-j phi}) / 2,
    nu = (1 - g e^{j phi}) / 2"""
    g, phi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
    return complex((1 + g * np.exp(-1j * phi)) / 2), complex((1 - g * np.exp(1j * phi)) / 2)


def rx_impair(x, mu=1.0, nu=0.0, dc=0.0):
    """out = mu x + nu conj(x) + dc in float32: a = x mu and b = conj(x) nu by rule 2, then (a + b) + dc per component"""
    v = widen(x)
    xr, xi = v[:, 0], v[:, 1]
    mr, mi, nr, ni = f32(np.real(mu)), f32(np.imag(mu)), f32(np.real(nu)), f32(np.imag(nu))
    with np.errstate(over="ignore", invalid="ignore"):
        ar, ai = fma32(-xi, mi, xr * mr), fma32(xi, mr, xr * mi)
        br, bi = fma32(xi, ni, xr * nr), fma32(-xi, nr, xr * ni)
        out = np.stack([(ar + br) + f32(np.real(dc)), (ai + bi) + f32(np.imag(dc))], axis=1).astype(np.float32)
    return np.ascontiguousarray(out).view(np.complex64).reshape(-1)
