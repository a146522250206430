"""NUMERICS.md rules 27 and 28 restated on the host: what wifirx_irs_taps_multi and wifirx_irs_sweep_multi (wr_irs.hip, wr_irs_sweep.hip)
compute, value for value.

Built on tests/irs_ref.py (rule 25) and tests/irs_sweep_ref.py (rule 26): antenna m of rule 27 IS rule 25 on the scatter row
(w_a[m], w_b, w_d[m]) with the line-of-sight values (A_m, B, D_m), so the restatement assembles those rows and calls
irs_ref.irs_taps once per antenna; the Philox draws of the antennas m >= 1 are made here from tests/channel_ref.py's Philox.
Rule 28 runs irs_sweep_ref's chain per antenna and adds the powers in ascending rho = m L + l.  Of the product only
wifirx.irs.PHASES is used, rule 25's table of the eight phases (tests/irs_ref.py leans on the same module for the argmax), to
turn antenna 0's codes into the phases of the other antennas."""
import math

import numpy as np

import channel_ref as cr
import irs_ref
import irs_sweep_ref as sr
from wifirx import irs

F32 = np.float32
MAX_ANT = 8


def counter_l(l, m):
    """counter word 2 of antenna m's draws: l for antenna 0, l + 16 ((m + 1) >> 1) for the others"""
    return l + 16 * ((m + 1) >> 1)


def words(m):
    """which two of the draw's four words antenna m takes: (x, y) for antenna 0 and the odd ones, (z, w) for the even ones"""
    return (0, 1) if (m == 0 or m & 1) else (2, 3)


def draws(n_sets, L, N, M, seed):
    """the Philox scatter: w_a complex64 [M, n_sets, L, N], w_b [n_sets, L, N], w_d [M, n_sets, L]"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    wa0, wb, wd0 = irs_ref.draws(n_sets, L, N, seed)
    wa, wd = [wa0], [wd0]
    r, l, n = np.meshgrid(np.arange(n_sets, dtype=np.uint32), np.arange(L, dtype=np.uint32), np.arange(N, dtype=np.uint32),
                          indexing="ij")
    two = np.full(n.shape, 2, np.uint32)
    for m in range(1, M):
        i, j = words(m)
        lm = counter_l(l, m).astype(np.uint32)
        d = cr.philox4x32_10(n, r, lm, two, k0, k1)
        wa.append(irs_ref.cplx(*irs_ref.gauss(d[i], d[j])))
        d = cr.philox4x32_10(np.full(r[:, :, 0].shape, irs_ref.DIRECT, np.uint32), r[:, :, 0], lm[:, :, 0], two[:, :, 0], k0, k1)
        wd.append(irs_ref.cplx(*irs_ref.gauss(d[i], d[j])))
    return np.stack(wa), wb, np.stack(wd)


def rows(wa, wb, wd):
    """scatter rows of rule 27 from w_a [M, R, N], w_b [R, N], w_d [M, R]: complex64 [R, (M + 1) N + M]"""
    M = wa.shape[0]
    return np.concatenate([wa[m] for m in range(M)] + [wb, np.stack([wd[m] for m in range(M)], axis=1)], axis=1).astype(np.complex64)


def antenna_rows(scatter, M, N, m):
    """rule 25's rows (w_a[m], w_b, w_d[m]) [n_scatter, 2 N + 1] out of rule 27's"""
    s = np.asarray(scatter, dtype=np.complex64)
    return np.ascontiguousarray(np.concatenate([s[:, m * N:(m + 1) * N], s[:, M * N:(M + 1) * N], s[:, (M + 1) * N + m, None]], axis=1))


def scene(pdp, los_b2r, los_b2u):
    pdp = np.asarray(pdp, dtype=F32).reshape(-1)
    A = np.asarray(los_b2r, dtype=np.complex64)
    A = A[None] if A.ndim == 1 else A
    D = None if los_b2u is None else np.asarray(los_b2u, dtype=np.complex64).reshape(-1)
    return pdp, A, D


def given(n_sets, L, N, M, scatter, seed):
    """the scatter rows the call reads: the given ones, or the Philox draws laid out as one row per (r, l)"""
    if scatter is not None:
        return np.asarray(scatter, dtype=np.complex64)
    wa, wb, wd = draws(n_sets, L, N, M, seed)
    return rows(wa.reshape(M, n_sets * L, N), wb.reshape(n_sets * L, N), wd.reshape(M, n_sets * L))


def irs_taps_multi(n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, gain=1.0, k_factor=0.0, direct_gain=1.0, psi=None, align_bits=0,
                   scatter=None, seed=0, elems=None):
    """WifiRx.irs_taps_multi restated.  los_b2r [M, N], los_b2u [M]; scatter: None (Philox) or [n_scatter, (M + 1) N + M];
    elems: the elements [n_sets, L, M + 1, N] to use in place of the mix.  Returns a dict: taps [M, n_sets, L] complex64, elems
    [n_sets, L, M + 1, N] complex64, direct [M, n_sets, L] complex64, codes [n_sets, N] uint8 or None."""
    pdp, A, D = scene(pdp, los_b2r, los_b2u)
    M, N, L = A.shape[0], A.shape[1], pdp.size
    if not 1 <= M <= MAX_ANT:
        raise ValueError("1..8 antennas")
    s = given(n_sets, L, N, M, scatter, seed)
    kw = dict(gain=gain, k_factor=k_factor, direct_gain=direct_gain)
    out, codes = [], None
    for m in range(M):
        el = None if elems is None else np.stack([np.asarray(elems)[:, :, m], np.asarray(elems)[:, :, M]], axis=2)
        ph = dict(psi=psi)
        if align_bits and m == 0:
            ph = dict(align_bits=align_bits)                      # the genie of the reference antenna decides ...
        elif align_bits:
            ph = dict(psi=irs.PHASES[codes.astype(np.intp) << (3 - align_bits)])       # ... and every antenna uses its codes
        o = irs_ref.irs_taps(n_sets, pdp, A[m], los_r2u, None if D is None else D[m], scatter=antenna_rows(s, M, N, m), elems=el,
                             **ph, **kw)
        if m == 0:
            codes = o["codes"]
        out.append(o)
    el = np.stack([o["elems"][:, :, 0] for o in out] + [out[0]["elems"][:, :, 1]], axis=2)
    for o in out:                                                 # one surface-to-user leg
        assert np.array_equal(o["elems"][:, :, 1].view(np.uint32), out[0]["elems"][:, :, 1].view(np.uint32))
    return {"taps": np.stack([o["taps"] for o in out]), "elems": el, "direct": np.stack([o["direct"] for o in out]), "codes": codes}


def power_sum(q):
    """P = q_0 + q_1 + ... in ascending rho from q_0: q [n_sets, M L, K] float32 -> [n_sets, K]"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = q[:, 0]
        for rho in range(1, q.shape[1]):
            p = p + q[:, rho]
    return p


def irs_sweep_multi(n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, codebook, gain=1.0, k_factor=0.0, direct_gain=1.0,
                    scatter=None, seed=0, elems=None):
    """WifiRx.irs_sweep_multi restated.  Returns a dict: taps [M, n_sets, L] complex64 (the winner's), best [n_sets] uint16, power
    [n_sets, K] float32, all_taps [M, n_sets, L, K] complex64, elems and direct as irs_taps_multi."""
    pdp, A, D = scene(pdp, los_b2r, los_b2u)
    M, N, L = A.shape[0], A.shape[1], pdp.size
    base = irs_taps_multi(n_sets, pdp, A, los_r2u, D, gain=gain, k_factor=k_factor, direct_gain=direct_gain,
                          psi=np.ones(N, np.complex64), scatter=scatter, seed=seed, elems=elems)
    scale = np.array([F32(math.sqrt(float(p)) * float(F32(gain))) for p in pdp], F32)
    c_re, c_im = sr.coefficients(codebook)
    el = base["elems"]
    b = irs_ref.parts(el[:, :, M])
    t_re, t_im = [], []
    for m in range(M):
        Am = sr.interleave(*irs_ref.mul(irs_ref.parts(el[:, :, m]), b))
        hd = irs_ref.parts(base["direct"][m])
        with np.errstate(invalid="ignore", over="ignore"):
            t_re.append((hd[0][..., None] + sr.chain(Am, c_re)) * scale[None, :, None])
            t_im.append((hd[1][..., None] + sr.chain(Am, c_im)) * scale[None, :, None])
    t_re, t_im = np.stack(t_re), np.stack(t_im)                   # [M, n_sets, L, K]
    with np.errstate(invalid="ignore", over="ignore"):
        q = t_re * t_re + t_im * t_im                             # two products and one add, each rounded
    power = power_sum(np.moveaxis(q, 0, 1).reshape(n_sets, M * L, -1))       # rho = m L + l
    best = sr.winner(power)
    pick = best.astype(np.intp)[None, :, None, None]
    taps = irs_ref.cplx(np.take_along_axis(t_re, pick, 3)[..., 0], np.take_along_axis(t_im, pick, 3)[..., 0])
    return {"taps": taps, "best": best, "power": power, "all_taps": irs_ref.cplx(t_re, t_im), "elems": el, "direct": base["direct"]}
