"""NUMERICS.md rule 25 restated on the host: what wifirx_irs_taps (wr_irs.hip) computes, value for value.

Everything is NumPy float32 on separate real and imaginary parts, plain products and sums (rule 17's ch_mul / ch_add), on top of
tests/channel_ref.py's Philox and Box-Muller.  With given scatter the restatement is bit-exact; with Philox scatter the
elements use NumPy's float32 log / sqrt / sin / cos where the device has its own, so they agree to rule 17's 1e-5, and
`elems` lets a caller feed the device's own elements into the rest of the chain, which is exact again."""
import math

import numpy as np

import channel_ref as cr
from wifirx import irs

F32 = np.float32
H = F32(0.70710678118654752)
DIRECT = 0xFFFFFFFF


def gauss(ua, ub):
    """rule 17's Box-Muller with h = sqrt(1/2): the parts of one complex Gaussian of variance 1"""
    with np.errstate(divide="ignore"):
        r = np.sqrt(F32(-2.0) * np.log(cr.u01(ua)))
    ang = cr.TWO_PI_F * cr.u01(ub)
    return (H * r) * np.cos(ang), (H * r) * np.sin(ang)


def draws(n_sets, L, N, seed):
    """the Philox scatter: (w_a, w_b) complex64 [n_sets, L, N] and w_d complex64 [n_sets, L]"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r, l, n = np.meshgrid(np.arange(n_sets, dtype=np.uint32), np.arange(L, dtype=np.uint32), np.arange(N, dtype=np.uint32),
                          indexing="ij")
    d = cr.philox4x32_10(n, r, l, np.full(n.shape, 2, np.uint32), k0, k1)
    wa, wb = cplx(*gauss(d[0], d[1])), cplx(*gauss(d[2], d[3]))
    r2, l2 = r[:, :, 0], l[:, :, 0]
    d = cr.philox4x32_10(np.full(r2.shape, DIRECT, np.uint32), r2, l2, np.full(r2.shape, 2, np.uint32), k0, k1)
    return wa, wb, cplx(*gauss(d[0], d[1]))


def cplx(re, im):
    out = np.empty(np.shape(re), np.complex64)
    out.real, out.imag = re, im
    return out


def parts(z):
    z = np.asarray(z, dtype=np.complex64)
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def mul(a, b):
    """ch_mul on (re, im) pairs of float32 arrays"""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def rician(k_factor):
    """(a_los, a_nlos) as the host forms them: in double from the float32 K, rounded once; K = 0: None (neither is applied)"""
    k = float(F32(k_factor))
    if k == 0.0:
        return None
    return F32(math.sqrt(k / (k + 1.0))), F32(math.sqrt(1.0 / (k + 1.0)))


def mix(los, w, co):
    """a_los * los + a_nlos * w per part; co = None: w itself"""
    if co is None:
        return w
    return co[0] * los[0] + co[1] * w[0], co[0] * los[1] + co[1] * w[1]


def wave_sum(p):
    """the rule's sum over the last axis (N): lane i of 64 adds its elements n = i, i + 64, ... in ascending n from its first
    product (a lane without an element holds +0), then the butterfly over lane xor 32, 16, 8, 4, 2, 1"""
    N = p.shape[-1]
    passes = -(-N // 64)
    pad = np.zeros(p.shape[:-1] + (passes * 64,), F32)
    pad[..., :N] = p
    pad = pad.reshape(p.shape[:-1] + (passes, 64))
    have = (np.arange(passes * 64) < N).reshape(passes, 64)
    acc = pad[..., 0, :].copy()
    for k in range(1, passes):
        acc = np.where(have[k], acc + pad[..., k, :], acc)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ m]
    assert (acc.view(np.uint32) == acc[..., :1].view(np.uint32)).all(), "the butterfly is symmetric"
    return acc[..., 0]


def irs_taps(n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, gain=1.0, k_factor=0.0, direct_gain=1.0, psi=None, align_bits=0,
             scatter=None, seed=0, elems=None):
    """WifiRx.irs_taps restated.  scatter: None (Philox) or [n_scatter, 2 N + 1]; psi: [N] or [n_psi_sets, N]; elems: the
    elements [n_sets, L, 2, N] to use in place of the mix (then only the direct path is drawn or read).  Returns a dict:
    taps [n_sets, L] complex64, elems [n_sets, L, 2, N] complex64, direct [n_sets, L] complex64 (h_d), codes [n_sets, N] uint8
    or None."""
    pdp = np.asarray(pdp, dtype=F32).reshape(-1)
    L, N = pdp.size, np.asarray(los_b2r).size
    scale = np.array([F32(math.sqrt(float(p)) * float(F32(gain))) for p in pdp], F32)
    co = rician(k_factor)
    dg = F32(direct_gain)
    if scatter is not None:
        s = np.asarray(scatter, dtype=np.complex64)
        row = (np.arange(n_sets)[:, None] * L + np.arange(L)[None, :]) % s.shape[0]
        wa, wb, wd = s[row, :N], s[row, N:2 * N], s[row, 2 * N]
    elif elems is None or dg != 0:
        wa, wb, wd = draws(n_sets, L, N, seed)
    if elems is None:
        a = mix(parts(los_b2r), parts(wa), co)
        b = mix(parts(los_r2u), parts(wb), co)
    else:
        e = np.asarray(elems, dtype=np.complex64)
        a, b = parts(e[:, :, 0, :]), parts(e[:, :, 1, :])
    if dg == 0:
        hd = (np.zeros((n_sets, L), F32), np.zeros((n_sets, L), F32))
    else:
        v = mix(parts(np.complex64(0 if co is None else los_b2u)), parts(wd), co)
        hd = (dg * v[0], dg * v[1])
    codes = None
    if align_bits:
        e0 = mul((a[0][:, 0], a[1][:, 0]), (b[0][:, 0], b[1][:, 0]))             # tap 0: [n_sets, N]
        codes = np.stack([irs.align_codes(e0[0][r], e0[1][r], hd[0][r, 0], hd[1][r, 0], align_bits) for r in range(n_sets)])
        k = codes.astype(np.intp) << (3 - align_bits)
        ph = (irs.PHASES_RE[k][:, None, :], irs.PHASES_IM[k][:, None, :])
    else:
        q = np.asarray(psi, dtype=np.complex64)
        q = q[None] if q.ndim == 1 else q
        q = q[np.arange(n_sets) % q.shape[0]]
        ph = (np.ascontiguousarray(q.real)[:, None, :], np.ascontiguousarray(q.imag)[:, None, :])
    p = mul(mul(a, ph), b)
    h = (hd[0] + wave_sum(p[0]), hd[1] + wave_sum(p[1]))
    el = np.empty((n_sets, L, 2, N), np.complex64)
    el[:, :, 0, :], el[:, :, 1, :] = cplx(*a), cplx(*b)
    return {"taps": cplx(h[0] * scale, h[1] * scale), "elems": el, "direct": cplx(*hd), "codes": codes}


def bound(hd, a, b):
    """the derived distance of rule 25 between the float32 chain and its float64 definition, per tap: the sum depth
    c(N) = ceil(N / 64) + 6 times 2^-24 times (|h_d| + sum_n |a_n| |b_n|); a, b [..., N], hd [...]"""
    N = np.shape(a)[-1]
    c = -(-N // 64) + 6
    return c * 2.0 ** -24 * (np.abs(hd) + (np.abs(a) * np.abs(b)).sum(axis=-1))
