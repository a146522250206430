"""The host side of the reflecting-surface channel (wifirx_irs_taps, NUMERICS.md rule 25; wifirx_irs_sweep, rule 26;
wifirx_irs_estimate, rule 29): the line-of-sight geometry the calls take as input, fixed phase configurations, beam-training
codebooks, pilot configurations and element groups for them, and the configuration object of ``block.channel_model(irs=...)``.

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


def los(irs_scale, irs_pos, ap_pos, user_pos, antennas=None):
    """The line-of-sight part of the three links for one AP antenna and one user, in float64: (b2r [N], r2u [N], b2u),
    N = irs_scale^2.  The AP and the user are single antennas (steering vector 1), so the AP -> surface link is the conjugate
    of the surface's steering vector towards the AP, the surface -> user link the steering vector of the direction from the
    user, and the direct link is 1.

    antennas = M (an int, 1..8): the AP is a uniform linear array of M antennas half a wavelength apart along x, the
    reference's genLoS with antennaNum = M, and the result is (b2r [M, N], r2u [N], b2u [M]):
    b2r[m, n] = exp(j pi m ux) b2r_single[n] and b2u[m] = exp(j pi m ux'), ux the x direction cosine from the surface to the AP
    and ux' the one from the user to the AP.  Antenna 0 is the single-antenna result."""
    s = int(irs_scale)
    if s < 1:
        raise ValueError("irs_scale must be >= 1")
    b2r = np.conj(_steer(s, _direction(ap_pos, irs_pos)))
    r2u = _steer(s, _direction(irs_pos, user_pos))
    if antennas is None:
        return b2r, r2u, complex(1.0)
    m = int(antennas)
    if not 1 <= m <= 8:
        raise ValueError("antennas must be 1..8")
    ula = lambda ux: np.exp(1j * math.pi * ux * np.arange(m))
    return ula(_direction(ap_pos, irs_pos)[0])[:, None] * b2r[None, :], r2u, ula(_direction(ap_pos, user_pos)[0])


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


def quantize(psi, bits):
    """Every phase of `psi` (complex, any shape) moved to the nearest of the 2^B table phases: rule 25's argmax on conj(psi)
    (code c maximises Re(conj(psi) C_c), the lowest c at a tie), so the result is exact and needs no atan2.  complex64."""
    p = np.asarray(psi, dtype=np.complex64)
    codes = align_codes(p.real, -p.imag, 0, 0, bits)
    return PHASES[codes.astype(np.intp) << (3 - bits)]


def dft_codebook(scale, los_b2r=None, over=1, bits=0):
    """A beam-training codebook of M^2 steering patterns for the scale x scale surface, M = over * scale beams per axis: entry
    k = i M + j points at the direction cosines (u_i, u_j), u_i = -1 + 2 i / M, after undoing the AP -> surface leg:
    psi_{k,n} = conj(A_n) / |A_n| exp(-j pi (u_i ix + u_j iy)) for element n = ix * scale + iy (the order of :func:`los`),
    A = los_b2r (None: 1).  over = 1 is the orthogonal DFT grid; over = 2 halves the scalloping loss between beams.
    bits > 0: quantised to a B-bit surface by :func:`quantize`.  complex64 [M^2, N]."""
    s, o = int(scale), int(over)
    if s < 1 or o < 1:
        raise ValueError("scale and over must be >= 1")
    m = o * s
    ix, iy = np.divmod(np.arange(s * s), s)
    u = -1.0 + 2.0 * np.arange(m) / m
    ui, uj = np.repeat(u, m), np.tile(u, m)
    cb = np.exp(-1j * math.pi * (ui[:, None] * ix[None, :] + uj[:, None] * iy[None, :]))
    if los_b2r is not None:
        a = np.asarray(los_b2r, dtype=np.complex128).reshape(-1)
        if a.size != s * s or not (np.abs(a) > 0).all():
            raise ValueError("los_b2r must hold scale^2 values that are not zero")
        cb = cb * (np.conj(a) / np.abs(a))[None, :]
    cb = cb.astype(np.complex64)
    return quantize(cb, bits) if bits else cb


def traverse_codebook(scale, interval, irs_pos, ap_pos, accuracy=10, freq=5e9, bits=0):
    """The grid of the reference's controller ("IRS Traverse" in gnu_radio/IRS_tranceiver.grc, the phase formula also in
    gnu_radio/IRS_AP.grc), written from the formula: theta_i, phi_j = linspace(-pi/2, pi/2, accuracy), entry k = i * accuracy + j,
    element n = ix * scale + iy at (x, y) = (irs_pos[0] + ix * interval, irs_pos[1] + iy * interval), D_n its distance to the
    AP, and psi_{k,n} = exp(j (2 pi freq / 3e8) (D_n - sin(theta) cos(phi) y_n - sin(theta) sin(phi) x_n)); at theta = 0 the
    formula's other branch, D_n - sin(phi) x_n.  bits > 0: quantised by :func:`quantize`.  complex64 [accuracy^2, N]."""
    s, acc = int(scale), int(accuracy)
    if s < 1 or acc < 1:
        raise ValueError("scale and accuracy must be >= 1")
    ix, iy = np.divmod(np.arange(s * s), s)
    x = float(irs_pos[0]) + ix * float(interval)
    y = float(irs_pos[1]) + iy * float(interval)
    dist = np.sqrt((x - float(ap_pos[0])) ** 2 + (y - float(ap_pos[1])) ** 2 + (float(irs_pos[2]) - float(ap_pos[2])) ** 2)
    wave = 2.0 * math.pi * float(freq) / 3e8
    grid = np.linspace(-math.pi / 2, math.pi / 2, acc)
    cb = np.empty((acc * acc, s * s), np.complex128)
    for i, th in enumerate(grid):
        for j, ph in enumerate(grid):
            if th != 0:
                pha = wave * (dist - math.sin(th) * math.cos(ph) * y - math.sin(th) * math.sin(ph) * x)
            else:
                pha = wave * (dist - math.sin(ph) * x)
            cb[i * acc + j] = np.exp(1j * pha)
    cb = cb.astype(np.complex64)
    return quantize(cb, bits) if bits else cb


def dft_pilots(n_groups):
    """The pilot configurations of a least-squares channel estimate (wifirx_irs_estimate, NUMERICS.md rule 29): T = G + 1 slots
    for G groups, pilot[t][g] = exp(-2 pi i t (g + 1) / (G + 1)), columns 1..G of the (G + 1)-point DFT matrix (the reference's
    Channel.DFT_matrix up to its 1 / sqrt(J)); column 0, the constant 1, is the direct path's and stays with the estimator.  The
    columns are orthogonal: sum_t conj(p_j) p_j' = T delta.  Formed in float64 and rounded once.  complex64 [G + 1, G]."""
    g = int(n_groups)
    if not 1 <= g <= 1023:
        raise ValueError("n_groups must be 1..1023")
    t, j = np.arange(g + 1)[:, None], np.arange(1, g + 1)[None, :]
    return np.exp(-2j * math.pi * ((t * j) % (g + 1)) / (g + 1)).astype(np.complex64)


def hadamard_pilots(n_groups):
    """Pilot configurations a 1-bit surface can realise: columns 1..G of the Sylvester-Hadamard matrix of order
    T = 2^ceil(log2(G + 1)), entries +-1 (column 0, all ones, is the direct path's).  Orthogonal as :func:`dft_pilots`.
    complex64 [T, G]."""
    g = int(n_groups)
    if not 1 <= g <= 1023:
        raise ValueError("n_groups must be 1..1023")
    t = 1 << g.bit_length()                                   # 2^ceil(log2(G + 1))
    i, j = np.arange(t)[:, None], np.arange(1, g + 1)[None, :]
    bits = i & j
    par = np.zeros_like(bits)
    while bits.any():
        par ^= bits & 1
        bits = bits >> 1
    return (1.0 - 2.0 * par).astype(np.complex64)


def groups(scale, c):
    """The reference's clustering (clustered_SV_channel, cluster_cale = c): c x c neighbouring elements of the scale x scale
    surface share one phase.  Element n = ix * scale + iy belongs to group (ix // c) * (scale // c) + iy // c; c must divide
    scale.  uint16 [scale^2], with (scale // c)^2 groups."""
    s, c = int(scale), int(c)
    if s < 1 or c < 1 or s % c:
        raise ValueError("c must divide scale")
    ix, iy = np.divmod(np.arange(s * s), s)
    return ((ix // c) * (s // c) + iy // c).astype(np.uint16)


def est_scale(n_pilots, sigma=0.0, mmse=False):
    """kappa of wifirx_irs_estimate as float32: 1 / T (least squares), or with mmse 1 / (T + sigma^2), the reference's
    Channel.CH_est (1 / (1 + sigma2) behind unitary pilots) for coefficients of variance 1."""
    t = int(n_pilots)
    if t < 1:
        raise ValueError("n_pilots must be >= 1")
    return F32(1.0 / (t + float(sigma) ** 2)) if mmse else F32(1.0 / t)


def row_weights(antennas, taps, tap=None, ant=None):
    """The row weights of wifirx_irs_optimize_weighted (NUMERICS.md rule 31) for M = antennas and L = taps: float32 [M L] with
    w_{m L + l} = ant[m] * tap[l], the product formed in float32, and ones where a factor is None.  ``tap`` holds L values
    (:func:`tap_weights`), ``ant`` M values (1 / sigma_m^2 for per-antenna noise weights)."""
    m, l = int(antennas), int(taps)
    if m < 1 or l < 1:
        raise ValueError("antennas and taps must be >= 1")
    a = np.ones(m, F32) if ant is None else np.asarray(ant, dtype=F32).reshape(-1)
    t = np.ones(l, F32) if tap is None else np.asarray(tap, dtype=F32).reshape(-1)
    if a.size != m or t.size != l:
        raise ValueError("ant must hold one value per antenna and tap one value per tap")
    return np.ascontiguousarray((a[:, None] * t[None, :]).reshape(-1))


def tap_weights(taps, keep=1, penalty=0.0):
    """Weights over the L = taps taps of one antenna: ``keep`` ones followed by ``-penalty``.  keep=1, penalty=0 aligns tap 0
    alone and leaves the other taps incoherent; a positive penalty also lowers the energy of the later taps, which is what makes
    the notches.  float32 [L]."""
    l, k = int(taps), int(keep)
    if l < 1 or not 0 <= k <= l:
        raise ValueError("taps must be >= 1 and keep 0..taps")
    w = np.full(l, -float(penalty), F32)
    w[:k] = 1.0
    return w


@dataclass
class IrsConfig:
    """What ``block.channel_model(irs=...)`` needs to draw its taps from wifirx_irs_taps.  The surface is given either by its
    geometry (``scale`` and the three positions, through :func:`los`) or by the line-of-sight vectors themselves; the phases
    either by ``psi`` ([N] complex), by ``align_bits`` = 1..3 (aligned per draw), or by ``codebook`` ([K, N] complex, K <= 1024:
    trained per draw by wifirx_irs_sweep, NUMERICS.md rule 26; excludes the other two).  ``refresh``: the number of samples
    after which a new tap set is drawn (set index = stream time // refresh).  ``antennas`` = M (1..8): the AP is the array of
    ``los(antennas=M)`` (wifirx_irs_taps_multi / wifirx_irs_sweep_multi, NUMERICS.md rules 27 and 28); the line-of-sight
    vectors are then [M, N], [N] and [M], and the block has M output ports.  M = 1 is the single-antenna surface.

    ``pilots`` ([T, G] complex, T <= 1024, G <= min(N, 1023): :func:`dft_pilots`, :func:`hadamard_pilots`) trains the surface per
    draw from noisy channel estimates instead (wifirx_irs_estimate, NUMERICS.md rule 29; excludes ``psi``, ``align_bits`` and
    ``codebook``): the surface steps through the pilots, is observed in noise of standard deviation ``pilot_sigma``, and loads
    the ``pilot_bits``-bit codes decided from the de-spread estimate.  ``group`` ([N] uint16, :func:`groups`; None: G = N) puts
    several elements behind one phase; ``est_scale`` is the estimator's kappa (None: 1 / T, least squares).

    ``decision`` says how the codes are decided from the estimate: "ref" (the default: rule 29's decision on antenna 0, tap 0) or
    "joint" (wifirx_irs_optimize, NUMERICS.md rule 30: at most ``sweeps`` = 0..16 sweeps of coordinate ascent on the power summed
    over every antenna and tap, started from the "ref" codes).  "joint" requires ``pilots``.

    ``tap_weights`` ([L], L the length of ``pdp``) and ``ant_weights`` ([antennas]) put a signed weight on every row of the joint
    decision (wifirx_irs_optimize_weighted, NUMERICS.md rule 31: :func:`row_weights` of the two, ones where one is None).  Both
    need ``decision="joint"`` and finite values; with both None the decision is rule 30's."""
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
    codebook: np.ndarray | None = None
    antennas: int = 1
    pilots: np.ndarray | None = None
    pilot_sigma: float = 0.0
    group: np.ndarray | None = None
    pilot_bits: int = 2
    est_scale: float | None = None
    decision: str = "ref"
    sweeps: int = 4
    tap_weights: tuple | None = None
    ant_weights: tuple | None = None
    n_elems: int = field(init=False, default=0)

    def __post_init__(self):
        geometry = (self.scale, self.irs_pos, self.ap_pos, self.user_pos)
        self.antennas = int(self.antennas)
        if not 1 <= self.antennas <= 8:
            raise ValueError("antennas must be 1..8")
        multi = self.antennas > 1
        if self.los_b2r is None and self.los_r2u is None:
            if any(v is None for v in geometry):
                raise ValueError("give scale and the three positions, or the line-of-sight vectors")
            self.los_b2r, self.los_r2u, self.los_b2u = los(*geometry, antennas=self.antennas) if multi else los(*geometry)
        elif self.los_b2r is None or self.los_r2u is None:
            raise ValueError("los_b2r and los_r2u come together")
        self.los_r2u = np.asarray(self.los_r2u, dtype=np.complex64).reshape(-1)
        if multi:
            self.los_b2r = np.ascontiguousarray(np.asarray(self.los_b2r, dtype=np.complex64))
            if self.los_b2r.ndim != 2 or self.los_b2r.shape[0] != self.antennas:
                raise ValueError("los_b2r must be [antennas, N]")
            self.n_elems = self.los_b2r.shape[1]
            if self.los_b2u is not None:
                self.los_b2u = np.ascontiguousarray(np.asarray(self.los_b2u, dtype=np.complex64).reshape(-1))
                if self.los_b2u.size != self.antennas:
                    raise ValueError("los_b2u must hold one value per antenna")
        else:
            self.los_b2r = np.asarray(self.los_b2r, dtype=np.complex64).reshape(-1)
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
        if self.decision not in ("ref", "joint"):
            raise ValueError("decision must be ref or joint")
        self.sweeps = int(self.sweeps)
        if not 0 <= self.sweeps <= 16:
            raise ValueError("sweeps must be 0..16")
        if self.decision == "joint" and self.pilots is None:
            raise ValueError("decision=joint needs pilots")
        for name, n in (("tap_weights", self.pdp.size), ("ant_weights", self.antennas)):
            w = getattr(self, name)
            if w is None:
                continue
            if self.decision != "joint":
                raise ValueError("%s needs decision=joint" % name)
            w = np.asarray(w, dtype=np.float32).reshape(-1)
            if w.size != n or not np.isfinite(w).all():
                raise ValueError("%s must hold %d finite values" % (name, n))
            setattr(self, name, np.ascontiguousarray(w))
        if self.pilots is not None:
            if self.psi is not None or self.align_bits or self.codebook is not None:
                raise ValueError("pilots exclude psi, align_bits and codebook")
            pl = np.ascontiguousarray(np.asarray(self.pilots, dtype=np.complex64))
            if pl.ndim != 2 or not 1 <= pl.shape[0] <= 1024 or not 1 <= pl.shape[1] <= min(self.n_elems, 1023):
                raise ValueError("pilots must be [T, G] with 1 <= T <= 1024 and 1 <= G <= min(N, 1023)")
            if self.group is None:
                if pl.shape[1] != self.n_elems:
                    raise ValueError("without a group map the pilots hold one column per element")
            else:
                g = np.asarray(self.group).reshape(-1)
                if g.size != self.n_elems or (g < 0).any() or (g >= pl.shape[1]).any():
                    raise ValueError("group must hold one value below G per element")
                self.group = np.ascontiguousarray(g.astype(np.uint16))
            self.pilots, self.pilot_sigma, self.pilot_bits = pl, float(self.pilot_sigma), int(self.pilot_bits)
            if not (math.isfinite(self.pilot_sigma) and self.pilot_sigma >= 0.0):
                raise ValueError("pilot_sigma must be finite and not negative")
            if self.pilot_bits not in (1, 2, 3):
                raise ValueError("pilot_bits must be 1, 2 or 3")
            self.est_scale = float(est_scale(pl.shape[0]) if self.est_scale is None else self.est_scale)
            if not math.isfinite(self.est_scale):
                raise ValueError("est_scale must be finite")
        elif self.group is not None:
            raise ValueError("group comes with pilots")
        elif self.codebook is not None:
            if self.psi is not None or self.align_bits:
                raise ValueError("codebook excludes psi and align_bits")
            cb = np.ascontiguousarray(np.asarray(self.codebook, dtype=np.complex64))
            if cb.ndim != 2 or cb.shape[1] != self.n_elems or not 1 <= cb.shape[0] <= 1024:
                raise ValueError("codebook must be [K, N] with 1 <= K <= 1024")
            self.codebook = cb
        elif self.align_bits == 0:
            self.set_psi(self.psi)
        self.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        self.refresh = int(self.refresh)
        if self.refresh < 1:
            raise ValueError("refresh must be >= 1 sample")

    @property
    def row_weights(self):
        """float32 [antennas * taps] for wifirx_irs_optimize_weighted, or None when neither weight is given (rule 30)"""
        if self.tap_weights is None and self.ant_weights is None:
            return None
        return row_weights(self.antennas, self.pdp.size, tap=self.tap_weights, ant=self.ant_weights)

    def set_psi(self, psi):
        if psi is None:
            raise ValueError("psi is required when align_bits is 0")
        p = np.asarray(psi, dtype=np.complex64).reshape(-1)
        if p.size != self.n_elems:
            raise ValueError("psi must hold one value per element")
        self.psi = np.ascontiguousarray(p)
