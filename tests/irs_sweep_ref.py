"""NUMERICS.md rule 26 restated on the host: what wifirx_irs_sweep (wr_irs_sweep.hip) computes, value for value.

NumPy float32 on separate real and imaginary parts.  The elements, the direct path and the scales are tests/irs_ref.py's (rule
25); the chain is tests/detect_ref.fma32, one rounding per term, vectorised over rows and entries and sequential over the 2 N
floats of a row.  Nothing of the product is imported here."""
import math

import numpy as np

import irs_ref
from detect_ref import fma32

F32 = np.float32


def coefficients(codebook):
    """the two coefficient rows of every entry: (c_re, c_im) float32 [K, P], P = 2 N filled with +0 up to a multiple of 4;
    c_re[2n] = psi.re, c_re[2n+1] = -psi.im (the real sum), c_im[2n] = psi.im, c_im[2n+1] = psi.re (the imaginary sum)"""
    cb = np.asarray(codebook, dtype=np.complex64)
    K, N = cb.shape
    P = -(-2 * N // 4) * 4
    c_re, c_im = np.zeros((K, P), F32), np.zeros((K, P), F32)
    c_re[:, 0:2 * N:2], c_re[:, 1:2 * N:2] = cb.real, -cb.imag
    c_im[:, 0:2 * N:2], c_im[:, 1:2 * N:2] = cb.imag, cb.real
    return c_re, c_im


def interleave(e_re, e_im):
    """A[2n] = e_n.re, A[2n+1] = e_n.im over the last axis, filled with +0 up to a multiple of 4"""
    N = e_re.shape[-1]
    A = np.zeros(e_re.shape[:-1] + (-(-2 * N // 4) * 4,), F32)
    A[..., 0:2 * N:2], A[..., 1:2 * N:2] = e_re, e_im
    return A


def chain(A, c):
    """sum = fma(A[phi], c[phi], sum) from +0 over phi ascending: A [..., P], c [K, P] -> [..., K]"""
    acc = np.zeros(A.shape[:-1] + (c.shape[0],), F32)
    for phi in range(A.shape[-1]):
        acc = fma32(A[..., phi, None], c[:, phi], acc)
    return acc


def winner(power):
    """best = 0, top = -1; k ascending, replace on a strict power > top: power [n_sets, K] -> uint16 [n_sets]"""
    best = np.zeros(power.shape[0], np.uint16)
    top = np.full(power.shape[0], F32(-1.0), F32)
    for k in range(power.shape[1]):
        with np.errstate(invalid="ignore"):
            better = power[:, k] > top
        top = np.where(better, power[:, k], top)
        best = np.where(better, np.uint16(k), best)
    return best


def from_parts(e, hd, scale, codebook):
    """the rule from the element products on: e = (re, im) [n_sets, L, N], hd = (re, im) [n_sets, L], scale [L], codebook [K, N]
    -> dict taps [n_sets, L] complex64, best [n_sets] uint16, power [n_sets, K] float32, all_taps [n_sets, L, K] complex64"""
    c_re, c_im = coefficients(codebook)
    A = interleave(*e)
    with np.errstate(invalid="ignore", over="ignore"):
        t_re = (hd[0][..., None] + chain(A, c_re)) * scale[None, :, None]
        t_im = (hd[1][..., None] + chain(A, c_im)) * scale[None, :, None]
        q = t_re * t_re + t_im * t_im                          # two products and one add, each rounded
        power = q[:, 0]
        for l in range(1, q.shape[1]):
            power = power + q[:, l]
    best = winner(power)
    pick = best.astype(np.intp)[:, None, None]
    taps = irs_ref.cplx(np.take_along_axis(t_re, pick, 2)[..., 0], np.take_along_axis(t_im, pick, 2)[..., 0])
    return {"taps": taps, "best": best, "power": power, "all_taps": irs_ref.cplx(t_re, t_im)}


def irs_sweep(n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, codebook, gain=1.0, k_factor=0.0, direct_gain=1.0, scatter=None,
              seed=0, elems=None):
    """WifiRx.irs_sweep restated; `elems` as in irs_ref.irs_taps.  Adds "elems" and "direct" (rule 25's) to from_parts' dict."""
    pdp = np.asarray(pdp, dtype=F32).reshape(-1)
    N = np.asarray(los_b2r).size
    base = irs_ref.irs_taps(n_sets, pdp, los_b2r, los_r2u, los_b2u, gain=gain, k_factor=k_factor, direct_gain=direct_gain,
                            psi=np.ones(N, np.complex64), scatter=scatter, seed=seed, elems=elems)
    scale = np.array([F32(math.sqrt(float(p)) * float(F32(gain))) for p in pdp], F32)
    el = base["elems"]
    e = irs_ref.mul(irs_ref.parts(el[:, :, 0, :]), irs_ref.parts(el[:, :, 1, :]))
    out = from_parts(e, irs_ref.parts(base["direct"]), scale, codebook)
    out.update(elems=el, direct=base["direct"])
    return out


def bound(hd, a, b, scale):
    """rule 26's distance between the winner's taps and rule 25's taps for psi = codebook[best], per tap:
    (2 N + ceil(N / 64) + 20) 2^-24 s_l (|h_d| + sum_n |a_n| |b_n|); a, b [n_sets, L, N], hd [n_sets, L], scale [L]"""
    N = np.shape(a)[-1]
    c = 2 * N + -(-N // 64) + 20
    return c * 2.0 ** -24 * np.abs(scale)[None, :] * (np.abs(hd) + (np.abs(a) * np.abs(b)).sum(axis=-1))
