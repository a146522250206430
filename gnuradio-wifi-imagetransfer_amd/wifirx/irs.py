"""The host side of the reflecting-surface channel (wifirx_irs_taps, NUMERICS.md rule 25): the line-of-sight geometry the call
takes as input, fixed phase configurations for it, and the configuration object of ``block.channel_model(irs=...)``.

The model is the reference's (utils/SV_channel.py, utils/channel.py) for one AP antenna and one user: a square surface of
S x S elements half a wavelength apart in the x-y plane, far-field steering vectors, H = H_B2R diag(psi) H_R2U + H_B2U.
Nothing here needs a device."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
_H = F32(0.70710678118654752)
# C_k = exp(j 2 pi k / 8) as rule 25's float32 table; code c of a B-bit surface is PHASES[c << (3 - B)]
PHASES_RE = np.array([1, _H, 0, -_H, -1, -_H, 0, _H], F32)
PHASES_IM = np.array([0, _H, 1, _H, 0, -_H, -1, -_H], F32)
PHASES = (PHASES_RE + 1j * PHASES_IM).astype(np.complex64)


def _direction(frm, to):
    d = np.asarray(frm, dtype=np.float64) - np.asarray(to, dtype=np.float64)
    return d / math.sqrt(float(d @ d))


def _steer(scale, direction):
    """steering vector of the S x S surface for a unit direction: element n = ix * S + iy has phase pi (dx ix + dy iy)"""
    ix, iy = np.divmod(np.arange(scale * scale), scale)
    return np.exp(1j * math.pi * (direction[0] * ix + direction[1] * iy))


def los(irs_scale, irs_pos, ap_pos, user_pos):
    """The line-of-sight part of the three links for one AP antenna and one user, in float64: (b2r [N], r2u [N], b2u),
    N = irs_scale^2.  The AP and the user are single antennas (steering vector 1), so the AP -> surface link is the conjugate
    of the surface's steering vector towards the AP, the surface -> user link the steering vector of the direction from the
    user, and the direct link is 1."""
    s = int(irs_scale)
    if s < 1:
        raise ValueError("irs_scale must be >= 1")
    b2r = np.conj(_steer(s, _direction(ap_pos, irs_pos)))
    r2u = _steer(s, _direction(irs_pos, user_pos))
    return b2r, r2u, complex(1.0)


def _mul32(ar, ai, br, bi):
    """rule 17's ch_mul on float32 parts"""
    return ar * br - ai * bi, ar * bi + ai * br


def align_codes(er, ei, dr, di, bits):
    """rule 25's argmax: e = (er, ei) float32 arrays, the direct path (dr, di) float32 scalars -> uint8 codes.  Code c
    maximises Re(conj(d) e C_c), the lowest c at a tie; d == 0 aligns to the positive real axis."""
    if bits not in (1, 2, 3):
        raise ValueError("bits must be 1, 2 or 3")
    er, ei = np.asarray(er, F32), np.asarray(ei, F32)
    dr, di = F32(dr), F32(di)
    if not (dr == 0 and di == 0):
        er, ei = _mul32(dr, -di, er, ei)
    up = 3 - bits
    best = np.zeros(er.shape, np.uint8)
    top = _mul32(er, ei, PHASES_RE[0], PHASES_IM[0])[0]
    for c in range(1, 1 << bits):
        m = _mul32(er, ei, PHASES_RE[c << up], PHASES_IM[c << up])[0]
        better = m > top
        top = np.where(better, m, top)
        best = np.where(better, np.uint8(c), best)
    return best


def align(b2r, r2u, b2u, bits):
    """The one fixed B-bit configuration a controller would load from the geometry: rule 25's argmax on the given vectors
    (taken as complex64) -> (codes uint8 [N], psi complex64 [N])."""
    a = np.asarray(b2r, dtype=np.complex64).reshape(-1)
    b = np.asarray(r2u, dtype=np.complex64).reshape(-1)
    d = np.complex64(b2u)
    er, ei = _mul32(a.real, a.imag, b.real, b.imag)
    codes = align_codes(er, ei, d.real, d.imag, bits)
    return codes, PHASES[codes.astype(np.intp) << (3 - bits)]


def random_psi(n, bits, seed):
    """n random B-bit phases (complex64), drawn from `seed`"""
    if bits not in (1, 2, 3):
        raise ValueError("bits must be 1, 2 or 3")
    codes = np.random.default_rng(seed).integers(0, 1 << bits, int(n))
    return PHASES[codes << (3 - bits)]


@dataclass
class IrsConfig:
    """What ``block.channel_model(irs=...)`` needs to draw its taps from wifirx_irs_taps.  The surface is given either by its
    geometry (``scale`` and the three positions, through :func:`los`) or by the line-of-sight vectors themselves; the phases
    either by ``psi`` ([N] complex) or by ``align_bits`` = 1..3 (aligned per draw).  ``refresh``: the number of samples after
    which a new tap set is drawn (set index = stream time // refresh)."""
    scale: int | None = None
    irs_pos: tuple | None = None
    ap_pos: tuple | None = None
    user_pos: tuple | None = None
    los_b2r: np.ndarray | None = None
    los_r2u: np.ndarray | None = None
    los_b2u: complex | None = None
    k_factor: float = 0.0
    direct_gain: float = 1.0
    pdp: tuple = (1.0,)
    gain: float = 1.0
    psi: np.ndarray | None = None
    align_bits: int = 0
    seed: int = 0
    refresh: int = 1 << 16
    n_elems: int = field(init=False, default=0)

    def __post_init__(self):
        geometry = (self.scale, self.irs_pos, self.ap_pos, self.user_pos)
        if self.los_b2r is None and self.los_r2u is None:
            if any(v is None for v in geometry):
                raise ValueError("give scale and the three positions, or the line-of-sight vectors")
            self.los_b2r, self.los_r2u, self.los_b2u = los(*geometry)
        elif self.los_b2r is None or self.los_r2u is None:
            raise ValueError("los_b2r and los_r2u come together")
        self.los_b2r = np.asarray(self.los_b2r, dtype=np.complex64).reshape(-1)
        self.los_r2u = np.asarray(self.los_r2u, dtype=np.complex64).reshape(-1)
        self.n_elems = self.los_b2r.size
        if self.los_r2u.size != self.n_elems or not 1 <= self.n_elems <= 4096:
            raise ValueError("los_b2r and los_r2u must have one length of 1..4096 elements")
        self.k_factor, self.direct_gain, self.gain = float(self.k_factor), float(self.direct_gain), float(self.gain)
        if not (math.isfinite(self.k_factor) and self.k_factor >= 0.0):
            raise ValueError("k_factor must be finite and not negative")
        if not (math.isfinite(self.direct_gain) and math.isfinite(self.gain)):
            raise ValueError("direct_gain and gain must be finite")
        if self.direct_gain != 0.0 and self.los_b2u is None:
            raise ValueError("a direct path needs los_b2u")
        self.pdp = np.asarray(self.pdp, dtype=np.float32).reshape(-1)
        if not 1 <= self.pdp.size <= 16 or not (np.isfinite(self.pdp).all() and (self.pdp >= 0).all()):
            raise ValueError("pdp must hold 1..16 finite values that are not negative")
        self.align_bits = int(self.align_bits)
        if self.align_bits not in (0, 1, 2, 3):
            raise ValueError("align_bits must be 0..3")
        if self.align_bits == 0:
            self.set_psi(self.psi)
        self.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        self.refresh = int(self.refresh)
        if self.refresh < 1:
            raise ValueError("refresh must be >= 1 sample")

    def set_psi(self, psi):
        if psi is None:
            raise ValueError("psi is required when align_bits is 0")
        p = np.asarray(psi, dtype=np.complex64).reshape(-1)
        if p.size != self.n_elems:
            raise ValueError("psi must hold one value per element")
        self.psi = np.ascontiguousarray(p)
