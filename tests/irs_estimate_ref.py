"""NUMERICS.md rule 29 restated on the host: what wifirx_irs_estimate (wr_irs_estimate.hip) computes, value for value.

NumPy float32 on separate real and imaginary parts.  The elements, the direct path, the scales and the taps under given phases are
tests/irs_multi_ref.py's (rule 27); the noiseless observation is irs_multi_ref.irs_sweep_multi's "all_taps" on the group-expanded
pilots (rule 28's tap of entry t, and so rule 26's chain from tests/irs_sweep_ref.py); the de-spread runs irs_sweep_ref.chain
again, over t; the noise is tests/channel_ref.py's Philox through irs_ref.gauss, rule 17's Box-Muller.  Of the product only
wifirx.irs.align_codes and PHASES are used, as tests/irs_ref.py uses them.

`mutant` switches one deliberate mistake on, for tests/test_irs_estimate_ref.py's mutation tests: "conj" (the de-spread multiplies by
p, not conj(p)), "kappa" (the scale is left out), "direct" (no direct column: group g lands in column g), "group" (the map is taken
as the identity modulo G), "sigma" (given noise is added unscaled)."""
import numpy as np

import channel_ref as cr
import irs_multi_ref as mr
import irs_ref
import irs_sweep_ref as sr
from wifirx import irs

F32 = np.float32
NOISE_WORD = 3                                                    # counter word 3 of the observation noise
MUTANTS = ("conj", "kappa", "direct", "group", "sigma")


def group_map(group, N, G):
    """the group of every element as intp [N]; None is the identity and needs G = N"""
    if group is None:
        if G != N:
            raise ValueError("no group map: n_groups must be n_elems")
        return np.arange(N)
    g = np.asarray(group, dtype=np.uint16).reshape(-1).astype(np.intp)
    if g.size != N or (g >= G).any():
        raise ValueError("group must hold n_elems values below n_groups")
    return g


def expand(pilot, gm):
    """the pilots as codebook rows: [T, N], element n of slot t carries pilot[t][group[n]]"""
    return np.ascontiguousarray(np.asarray(pilot, dtype=np.complex64)[:, gm])


def noise_draws(n_sets, R, T, seed):
    """the Philox noise: w complex64 [n_sets, R, T] from words (x, y) of the counter (t, r, rho, 3)"""
    r, rho, t = np.meshgrid(np.arange(n_sets, dtype=np.uint32), np.arange(R, dtype=np.uint32), np.arange(T, dtype=np.uint32),
                            indexing="ij")
    d = cr.philox4x32_10(t, r, rho, np.full(t.shape, NOISE_WORD, np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return irs_ref.cplx(*irs_ref.gauss(d[0], d[1]))


def columns(pilot, mutant=None):
    """the de-spreading columns p [T, J]: column 0 the constant 1, column g + 1 pilot[:, g]"""
    pl = np.asarray(pilot, dtype=np.complex64)
    if mutant == "direct":
        return np.concatenate([pl, np.ones((pl.shape[0], 1), np.complex64)], axis=1)
    return np.concatenate([np.ones((pl.shape[0], 1), np.complex64), pl], axis=1)


def coefficients(p, mutant=None):
    """the two coefficient rows of every column: (c_re, c_im) float32 [J, P], P = 2 T filled up to a multiple of 4 with the zero
    terms of p = 0; c_re[2t] = p.re, c_re[2t+1] = p.im (the real sum of obs conj(p)), c_im[2t] = -p.im, c_im[2t+1] = p.re"""
    T, J = p.shape
    P = -(-2 * T // 4) * 4
    pr, pi = np.zeros((J, P // 2), F32), np.zeros((J, P // 2), F32)
    pr[:, :T], pi[:, :T] = p.real.T, p.imag.T
    if mutant == "conj":
        pi = -pi
    c_re, c_im = np.empty((J, P), F32), np.empty((J, P), F32)
    c_re[:, 0::2], c_re[:, 1::2] = pr, pi
    c_im[:, 0::2], c_im[:, 1::2] = -pi, pr                        # (-(+0) = -0: the zero term of the imaginary sum)
    return c_re, c_im


def despread(obs, pilot, kappa, mutant=None):
    """ghat [..., J] complex64 from obs [..., T]: one chain per part over obs.re, obs.im in ascending t, then one multiply"""
    c_re, c_im = coefficients(columns(pilot, mutant), mutant)
    A = sr.interleave(*irs_ref.parts(obs))
    with np.errstate(invalid="ignore", over="ignore"):
        re, im = sr.chain(A, c_re), sr.chain(A, c_im)
        if mutant != "kappa":
            re, im = F32(kappa) * re, F32(kappa) * im
    return irs_ref.cplx(re, im)


def decide(est, bits, blocked=False):
    """rule 25's argmax on row 0 of every set with the estimate: est [n_sets, R, J] -> codes uint8 [n_sets, G].  blocked: the
    direct path is blocked (direct_gain = 0), its estimate is not consulted and the codes align to the positive real axis"""
    re, im = irs_ref.parts(est[:, 0])
    hd = (np.zeros_like(re[:, 0]), np.zeros_like(im[:, 0])) if blocked else (re[:, 0], im[:, 0])
    return np.stack([irs.align_codes(re[r, 1:], im[r, 1:], hd[0][r], hd[1][r], bits) for r in range(est.shape[0])])


def irs_estimate(n_sets, pdp, los_b2r, los_r2u, los_b2u=None, *, pilots, group=None, sigma=0.0, est_scale=None, align_bits=0,
                 gain=1.0, k_factor=0.0, direct_gain=1.0, scatter=None, noise=None, seed=0, elems=None, mutant=None):
    """WifiRx.irs_estimate restated; `elems` as in irs_multi_ref.irs_taps_multi.  Returns a dict: obs [n_sets, R, T], x (the
    noiseless observation), est [n_sets, R, J] complex64, elems, direct, and with align_bits codes [n_sets, G] uint8, psi
    [n_sets, N] complex64 and taps [M, n_sets, L] complex64."""
    pdp, A, D = mr.scene(pdp, los_b2r, los_b2u)
    M, N, L = A.shape[0], A.shape[1], pdp.size
    pl = np.asarray(pilots, dtype=np.complex64)
    T, G = pl.shape
    R = M * L
    gm = group_map(group, N, G)
    kw = dict(gain=gain, k_factor=k_factor, direct_gain=direct_gain, scatter=scatter, seed=seed, elems=elems)
    sw = mr.irs_sweep_multi(n_sets, pdp, A, los_r2u, D, codebook=expand(pl, np.arange(N) % G if mutant == "group" else gm), **kw)
    x = np.ascontiguousarray(np.moveaxis(sw["all_taps"], 0, 1).reshape(n_sets, R, T))          # rho = m L + l
    obs = x
    sg = F32(sigma)
    if sg != 0:
        if noise is not None:
            w = np.asarray(noise, dtype=np.complex64)
            w = w[np.arange(n_sets * R) % w.shape[0]].reshape(n_sets, R, T)
        else:
            w = noise_draws(n_sets, R, T, seed)
        s = F32(1.0) if (mutant == "sigma" and noise is not None) else sg
        with np.errstate(invalid="ignore", over="ignore"):
            obs = irs_ref.cplx(x.real + s * w.real, x.imag + s * w.imag)
    kappa = F32(1.0 / T) if est_scale is None else F32(est_scale)
    est = despread(obs, pl, kappa, mutant)
    out = {"obs": obs, "x": x, "est": est, "elems": sw["elems"], "direct": sw["direct"]}
    if align_bits:
        codes = decide(est, align_bits, blocked=F32(direct_gain) == 0)
        psi = irs.PHASES[codes[:, gm].astype(np.intp) << (3 - align_bits)]
        taps = mr.irs_taps_multi(n_sets, pdp, A, los_r2u, D, psi=psi, **kw)["taps"]
        out.update(codes=codes, psi=psi, taps=taps)
    return out


def chain_bound(obs, kappa):
    """rule 29's distance between the float32 de-spread and its float64 value, per part, for pilots of modulus <= 1:
    (2 T + 2) 2^-24 |kappa| sum_t (|obs.re| + |obs.im|); obs [..., T] -> [...]"""
    o = np.asarray(obs, dtype=np.complex128)
    T = o.shape[-1]
    return (2 * T + 2) * 2.0 ** -24 * abs(float(kappa)) * (np.abs(o.real) + np.abs(o.imag)).sum(axis=-1)


def forward_bound(hd, e, scale_rows):
    """the same count for the observation chain of 2 N terms plus the add of h_d and the multiply by s_l, per part, for pilots of
    modulus <= 1: (2 N + 2) 2^-24 s (|h_d.re| + |h_d.im| + sum_n (|e.re| + |e.im|)); hd, scale_rows [...], e [..., N]"""
    e = np.asarray(e, dtype=np.complex128)
    hd = np.asarray(hd, dtype=np.complex128)
    N = e.shape[-1]
    return (2 * N + 2) * 2.0 ** -24 * np.abs(scale_rows) * (np.abs(hd.real) + np.abs(hd.imag) + (np.abs(e.real) + np.abs(e.imag)).sum(-1))


def truth(out, pdp, gain, gm, G, M):
    """what an exact estimator returns at sigma = 0 with orthogonal pilots, in float64: g [n_sets, R, J], column 0 = s_l h_d,
    column g + 1 = s_l sum_{n in g} e_n, from the restatement's own elements; also (e [n_sets, R, N], hd, s) in rows"""
    el = np.asarray(out["elems"], dtype=np.complex64)
    n_sets, L = el.shape[0], el.shape[1]
    ar, ai = irs_ref.parts(el[:, :, :M])
    br, bi = irs_ref.parts(el[:, :, M])
    er, ei = irs_ref.mul((ar, ai), (br[:, :, None], bi[:, :, None]))                        # float32 ch_mul: [n_sets, L, M, N]
    e = np.moveaxis(er.astype(np.float64) + 1j * ei.astype(np.float64), 2, 1).reshape(n_sets, M * L, -1)
    hd = np.moveaxis(np.asarray(out["direct"], dtype=np.complex128), 0, 1).reshape(n_sets, M * L)
    s1 = np.array([float(F32(np.sqrt(float(p)) * float(F32(gain)))) for p in np.asarray(pdp, F32).reshape(-1)])
    s = np.tile(s1, M)[None, :]
    g = np.zeros((n_sets, M * L, G + 1), np.complex128)
    g[..., 0] = s * hd
    for k in range(G):
        g[..., k + 1] = s * e[..., gm == k].sum(axis=-1)
    return g, e, hd, np.broadcast_to(s, hd.shape)
