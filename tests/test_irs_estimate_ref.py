"""NUMERICS.md rule 29 on the host: tests/irs_estimate_ref.py, the restatement of wifirx_irs_estimate, against
  * the reference's own estimator (Channel.CH_est over Channel.DFT_matrix pilots, recorded by tools/make_golden_irs_estimate.py);
  * the exact answer at sigma = 0 for DFT and Hadamard pilots, grouped and not, within the rule's two chain bounds added;
  * the genie's codes at sigma = 0 (G = N): at most 1 differing element in 1000;
  * the error variance sigma^2 / T of a least-squares estimate, and the independence of the noise from rule 27's draws;
  * the edges: one pilot, a zero s_0, a zero direct estimate, NaN pilots;
  * five mutants of the restatement, each caught by the check named for it (test_mutation_table prints the log kept as
    profiles/irs_estimate_mutations.txt).
Every check is a function check_*(mutant=None) that raises AssertionError; test_* runs it on the restatement, test_mutant_* expects
it to fail on the mutant."""
import math
import os

import numpy as np
import pytest

import irs_estimate_ref as er
import irs_multi_ref as mr
import irs_ref
from wifirx import irs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "irs_estimate_reference.npz")
U = 2.0 ** -24


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def scene(rng, M, N, L, n_scatter):
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    return crandn(rng, M, N), crandn(rng, N), crandn(rng, M), pdp, crandn(rng, n_scatter, (M + 1) * N + M)


def pilots_of(kind, G):
    return irs.dft_pilots(G) if kind == "dft" else irs.hadamard_pilots(G)


# ---- the reference's estimator ----

def test_reference_estimator_is_the_rule():
    """obs = sqrt(J) y_rx, p = sqrt(J) Pilot^T = wifirx.irs.dft_pilots(J - 1) behind the constant column, kappa = 1 / (J (1 + sigma2))
    give Channel.CH_est.  Bound per part: the chain's (2 T + 2) u kappa sum (|obs.re| + |obs.im|), and 2 u more of the same sum for
    the two roundings to float32 that the inputs take (obs and the pilots), u = 2^-24."""
    z = np.load(GOLDEN)
    worst = 0.0
    for J in (5, 17):
        pilot = z["Pilot_J%d" % J]
        pl = irs.dft_pilots(J - 1)
        p = np.concatenate([np.ones((J, 1)), pl.astype(np.complex128)], axis=1)
        assert np.abs(p.T / math.sqrt(J) - pilot).max() < 4 * U                 # the mapping of the pilots
        for A in (1, 4):
            tag = "J%d_A%d" % (J, A)
            for i, s2 in enumerate(z["sigma2"]):
                y, want = z["y_" + tag][i], z["Hest_" + tag][i]
                assert np.abs(z["H_" + tag][i] @ pilot + z["noise_" + tag][i] - y).max() < 1e-13
                obs = (math.sqrt(J) * y).astype(np.complex64)
                kappa = np.float32(1.0 / (J * (1.0 + s2)))
                assert kappa == irs.est_scale(J, math.sqrt(J * s2), mmse=True)    # 1 / (T + sigma^2), sigma^2 = J sigma2
                got = er.despread(obs, pl, kappa).astype(np.complex128)
                # the mapping in float64, then the float32 chain against it
                assert np.abs(float(kappa) * (math.sqrt(J) * y) @ p.conj() - want).max() < 1e-6
                assert np.abs((1.0 / (J * (1 + s2))) * (math.sqrt(J) * y) @ (math.sqrt(J) * pilot.T).conj() - want).max() < 8e-15
                bound = (er.chain_bound(obs, kappa) * (2 * J + 4) / (2 * J + 2))[:, None]
                for d in ((got - want).real, (got - want).imag):
                    assert (np.abs(d) <= bound).all()
                    worst = max(worst, float((np.abs(d) / bound).max()))
    print("reference estimator: largest difference / bound = %.3f" % worst)


# ---- exactness at sigma = 0 ----

def exact_case(kind, grouped, mutant=None, k_factor=3.0):
    """(est, ref64, g, bound) of one sigma = 0 scene: est the restatement's, g the exact coefficients in float64, ref64 what an
    exact de-spread of the exact observations gives with the pilots as rounded to complex64 (g itself when their columns are
    exactly orthogonal), bound per part = the de-spread chain's bound + kappa sum_t (both parts' forward bounds) = the two added"""
    M, L, n_sets = 2, 3, 3
    N, gmap, G = (16, irs.groups(4, 2), 4) if grouped else (7, None, 7)
    rng = np.random.default_rng(5 + N)
    a, b, d, pdp, sc = scene(rng, M, N, L, n_sets * L - 1)
    pl = pilots_of(kind, G)
    T = pl.shape[0]
    kappa = irs.est_scale(T)
    out = er.irs_estimate(n_sets, pdp, a, b, d, pilots=pl, group=gmap, sigma=0.0, est_scale=kappa, gain=1.3, k_factor=k_factor,
                          scatter=sc, mutant=mutant)
    gm = er.group_map(gmap, N, G)
    g, e, hd, s = er.truth(out, pdp, 1.3, gm, G, M)
    P = er.columns(pl).astype(np.complex128)
    ref64 = float(kappa) * np.einsum("jk,...k->...j", P.conj().T @ P, g)
    bound = (er.chain_bound(out["obs"], kappa) + 2.0 * er.forward_bound(hd, e, s))[..., None]
    return out["est"].astype(np.complex128), ref64, g, bound


def check_exact(kind, grouped, mutant=None):
    est, ref64, g, bound = exact_case(kind, grouped, mutant)
    J = g.shape[-1]
    # the pilots' columns are orthogonal up to their rounding to complex64: ref64 is g to that defect
    assert (np.abs(ref64 - g) <= 4 * J * U * np.abs(g).sum(axis=-1, keepdims=True)).all()
    worst = 0.0
    for d in ((est - ref64).real, (est - ref64).imag):
        assert (np.abs(d) <= bound).all(), float((np.abs(d) / bound).max())
        worst = max(worst, float((np.abs(d) / bound).max()))
    return worst


@pytest.mark.parametrize("kind", ["dft", "hadamard"])
@pytest.mark.parametrize("grouped", [False, True])
def test_exact_at_sigma_zero(kind, grouped):
    print("%s grouped=%s: largest difference / bound = %.3f" % (kind, grouped, check_exact(kind, grouped)))


def check_conjugate(mutant=None):
    check_exact("dft", False, mutant)                          # complex pilots: p in place of conj(p) lands on the mirrored column


def check_scale(mutant=None):
    check_exact("hadamard", False, mutant)                     # real pilots: only the scale can be wrong


def check_direct_column(mutant=None):
    est, ref64, g, bound = exact_case("hadamard", True, mutant)
    for d in ((est - ref64)[..., 0].real, (est - ref64)[..., 0].imag):     # column 0 is s_l h_d
        assert (np.abs(d) <= bound[..., 0]).all()
    assert (np.abs(g[..., 0]) > 100 * bound[..., 0]).any()


def check_group_map(mutant=None):
    check_exact("dft", True, mutant)                           # groups(4, 2) is not n % G


def check_given_noise_scaled(mutant=None):
    rng = np.random.default_rng(77)
    M, N, L, n_sets, sigma = 2, 5, 2, 3, np.float32(0.5)
    a, b, d, pdp, sc = scene(rng, M, N, L, 4)
    pl = irs.dft_pilots(N)
    w = crandn(rng, 5, pl.shape[0])                            # 5 rows for 12 (set, row) pairs: they wrap
    out = er.irs_estimate(n_sets, pdp, a, b, d, pilots=pl, sigma=sigma, scatter=sc, noise=w, mutant=mutant)
    rows = w[np.arange(n_sets * M * L) % 5].reshape(n_sets, M * L, -1)
    assert irs_ref.cplx(out["x"].real + sigma * rows.real, out["x"].imag + sigma * rows.imag).tobytes() == out["obs"].tobytes()
    quiet = er.irs_estimate(n_sets, pdp, a, b, d, pilots=pl, sigma=0.0, scatter=sc, noise=w, mutant=mutant)
    assert quiet["obs"].tobytes() == quiet["x"].tobytes() == out["x"].tobytes()       # sigma = 0: obs = x, the rows are not read


CHECKS = {"conj": check_conjugate, "kappa": check_scale, "direct": check_direct_column, "group": check_group_map,
          "sigma": check_given_noise_scaled}


@pytest.mark.parametrize("name", er.MUTANTS)
def test_check_passes_on_the_restatement(name):
    CHECKS[name]()


def test_mutant_conj_dropped():
    with pytest.raises(AssertionError):
        check_conjugate("conj")


def test_mutant_kappa_omitted():
    with pytest.raises(AssertionError):
        check_scale("kappa")


def test_mutant_direct_column_missing():
    with pytest.raises(AssertionError):
        check_direct_column("direct")


def test_mutant_group_map_ignored():
    with pytest.raises(AssertionError):
        check_group_map("group")


def test_mutant_sigma_not_applied_to_given_noise():
    with pytest.raises(AssertionError):
        check_given_noise_scaled("sigma")


# ---- the codes at sigma = 0 ----

@pytest.mark.parametrize("N,bits,n_sets", [(16, 2, 64), (16, 3, 64), (64, 2, 16), (64, 3, 16), (255, 2, 4), (255, 3, 4)])
def test_codes_at_sigma_zero_are_the_genie_s(N, bits, n_sets):
    """G = N, Rayleigh, (N + 1)-point DFT pilots, kappa = 1 / T: the codes decided from the estimate are the genie's, except where
    an element lies within the estimate's float32 error of a decision boundary: at most 1 element in 1000 (a condition)."""
    rng = np.random.default_rng(1000 * bits + N)
    a, b, d, pdp, sc = scene(rng, 1, N, 1, n_sets)
    kw = dict(k_factor=0.0, scatter=sc)
    out = er.irs_estimate(n_sets, pdp, a, b, d, pilots=irs.dft_pilots(N), sigma=0.0, align_bits=bits, **kw)
    genie = mr.irs_taps_multi(n_sets, pdp, a, b, d, align_bits=bits, **kw)
    differ = int((out["codes"] != genie["codes"]).sum())
    print("N = %d, B = %d: %d of %d codes differ" % (N, bits, differ, n_sets * N))
    assert differ * 1000 <= n_sets * N
    if differ == 0:
        assert out["taps"].tobytes() == genie["taps"].tobytes()


def test_blocked_direct_path_aligns_to_the_real_axis():
    """direct_gain = 0: the estimate of the direct path is the chain's rounding residue (not zero in both parts) and, with noise,
    noise; the rule does not consult it and aligns to the positive real axis, as rule 25's genie does with h_d = +0.  So at
    sigma = 0 the codes are the genie's here too, and with noise they are what align_codes gives against a zero direct path."""
    N, bits, n_sets = 64, 2, 16
    rng = np.random.default_rng(64)
    a, b, d, pdp, sc = scene(rng, 1, N, 1, n_sets)
    kw = dict(k_factor=0.0, direct_gain=0.0, scatter=sc)
    out = er.irs_estimate(n_sets, pdp, a, b, None, pilots=irs.dft_pilots(N), sigma=0.0, align_bits=bits, **kw)
    genie = mr.irs_taps_multi(n_sets, pdp, a, b, None, align_bits=bits, **kw)
    assert (out["est"][:, 0, 0] != 0).any()                     # the residue is there; it is not consulted
    differ = int((out["codes"] != genie["codes"]).sum())
    assert differ * 1000 <= n_sets * N
    if differ == 0:
        assert out["taps"].tobytes() == genie["taps"].tobytes()
    noisy = er.irs_estimate(n_sets, pdp, a, b, None, pilots=irs.dft_pilots(N), sigma=2.0, align_bits=bits, seed=5, **kw)
    re, im = irs_ref.parts(noisy["est"][:, 0])
    for r in range(n_sets):
        assert np.array_equal(noisy["codes"][r], irs.align_codes(re[r, 1:], im[r, 1:], 0.0, 0.0, bits))
    # with a direct path, however small, the estimate of it is the reference
    on = er.irs_estimate(n_sets, pdp, a, b, d, pilots=irs.dft_pilots(N), sigma=2.0, align_bits=bits, seed=5, **dict(kw, direct_gain=1e-3))
    assert (on["codes"] != noisy["codes"]).any()


# ---- the noise ----

def test_error_variance_is_sigma2_over_T():
    """orthogonal pilots, kappa = 1 / T: every |ghat - g|^2 is exponential with mean sigma^2 / T, so the mean over X coefficients
    has the relative standard deviation 1 / sqrt(X); 5 of them is the gate"""
    M, N, L, n_sets, sigma = 2, 15, 4, 16, 2.0
    rng = np.random.default_rng(3)
    a, b, d, pdp, sc = scene(rng, M, N, L, n_sets * L)
    pl = irs.dft_pilots(N)
    T = pl.shape[0]
    kw = dict(pilots=pl, est_scale=irs.est_scale(T), scatter=sc, seed=0xABCDEF)
    noisy = er.irs_estimate(n_sets, pdp, a, b, d, sigma=sigma, **kw)
    g = er.truth(noisy, pdp, 1.0, np.arange(N), N, M)[0]
    err = np.abs(noisy["est"].astype(np.complex128) - g) ** 2
    X = err.size
    assert X >= 2000
    ratio = err.mean() / (sigma ** 2 / T)
    print("error variance / (sigma^2 / T) = %.4f over %d coefficients" % (ratio, X))
    assert abs(ratio - 1.0) <= 5.0 / math.sqrt(X)


def test_noise_counters_never_meet_rule_27():
    M, L, n_sets, N = 2, 4, 64, 32                              # T = N: the noise and the scatter line up index for index
    seed = 0x1234567
    w = er.noise_draws(n_sets, M * L, N, seed).reshape(n_sets, M, L, N)
    wa, wb, wd = mr.draws(n_sets, L, N, M, seed)               # [M, n_sets, L, N], [n_sets, L, N], [M, n_sets, L]
    # word 3 is 3 here and 2 in every draw of rules 25 to 28 (0 the channel's noise, 1 the fader): no counter is shared
    assert er.NOISE_WORD == 3
    corr = lambda x, y: abs(np.vdot(x.ravel(), y.ravel())) / math.sqrt(np.vdot(x, x).real * np.vdot(y, y).real)
    pairs = {"w_a": (np.moveaxis(w, 1, 0), wa), "w_b": (w[:, 0], wb), "w_d": (np.moveaxis(w[..., 0], 1, 0), wd)}
    for name, (x, y) in pairs.items():
        assert x.shape == y.shape
        c = corr(x.astype(np.complex128), y.astype(np.complex128))
        print("correlation of the noise with %s: %.4f (n = %d)" % (name, c, x.size))
        assert c < 5.0 / math.sqrt(x.size)
    assert abs(np.mean(np.abs(w) ** 2) - 1.0) < 5.0 / math.sqrt(w.size)          # variance 1
    assert not np.array_equal(w, er.noise_draws(n_sets, M * L, N, seed + 1).reshape(w.shape))


# ---- the edges ----

def test_one_pilot():
    rng = np.random.default_rng(9)
    a, b, d, pdp, sc = scene(rng, 2, 3, 2, 4)
    pl = np.array([[0.6 - 0.8j]], np.complex64)               # T = 1, G = 1: 2 T = 2 is filled with two zero terms
    out = er.irs_estimate(2, pdp, a, b, d, pilots=pl, group=np.zeros(3, np.uint16), est_scale=0.5, align_bits=2, scatter=sc)
    obs = out["obs"][..., 0]
    assert np.array_equal(out["est"][..., 0], irs_ref.cplx(np.float32(0.5) * obs.real, np.float32(0.5) * obs.imag))
    want = obs.astype(np.complex128) * np.conj(np.complex128(pl[0, 0])) * 0.5
    assert np.abs(out["est"][..., 1] - want).max() < 1e-6 * np.abs(want).max()
    assert out["codes"].shape == (2, 1) and out["taps"].shape == (2, 2, 2)


def test_zero_first_tap_gives_code_zero():
    rng = np.random.default_rng(10)
    a, b, d, pdp, sc = scene(rng, 2, 16, 3, 6)
    pdp[0] = 0.0                                              # s_0 = 0: row 0 observes nothing, every estimate of it is zero
    out = er.irs_estimate(3, pdp, a, b, d, pilots=irs.hadamard_pilots(4), group=irs.groups(4, 2), align_bits=3, scatter=sc)
    assert (out["est"][:, 0] == 0).all() and (out["codes"] == 0).all()
    assert (out["psi"] == 1).all() and np.abs(out["taps"][:, :, 1:]).min() > 0


def test_zero_direct_estimate_aligns_to_the_real_axis():
    pl = irs.hadamard_pilots(7)                                # +-1: the sums below are exact
    g = np.array([3, -2, 1j, -1j, 1 + 1j, -1 - 1j, 2 - 1j], np.complex64)
    obs = (pl.astype(np.complex128) @ g.astype(np.complex128)).astype(np.complex64)[None, None, :]       # no direct path
    est = er.despread(obs, pl, np.float32(0.125))
    assert est[0, 0, 0] == 0 and np.array_equal(est[0, 0, 1:], g)
    for bits in (1, 2, 3):
        codes = er.decide(est, bits)[0]
        assert np.array_equal(codes, irs.align_codes(g.real, g.imag, 0.0, 0.0, bits))
        turned = g * irs.PHASES[codes.astype(np.intp) << (3 - bits)]
        assert (turned.real >= np.abs(turned) * math.cos(math.pi / (1 << bits)) - 1e-6).all()


def test_nan_pilots_do_not_crash():
    rng = np.random.default_rng(11)
    a, b, d, pdp, sc = scene(rng, 1, 4, 2, 2)
    pl = irs.dft_pilots(4).copy()
    pl[2, 1] = np.nan
    out = er.irs_estimate(2, pdp, a, b, d, pilots=pl, align_bits=2, scatter=sc)
    assert np.isnan(out["obs"][..., 2]).all() and np.isnan(out["est"]).all()
    assert (out["codes"] == 0).all() and np.isfinite(out["taps"]).all()       # a NaN never beats code 0


def test_pilot_helpers():
    for G in (1, 3, 4, 15, 16, 255):
        for pl in (irs.dft_pilots(G), irs.hadamard_pilots(G)):
            P = er.columns(pl).astype(np.complex128)
            T = P.shape[0]
            assert pl.dtype == np.complex64 and pl.shape[1] == G and np.abs(P.conj().T @ P - T * np.eye(G + 1)).max() < 4 * T * U
        assert irs.dft_pilots(G).shape[0] == G + 1
        h = irs.hadamard_pilots(G)
        assert h.shape[0] == 1 << math.ceil(math.log2(G + 1)) and (h.imag == 0).all() and (np.abs(h.real) == 1).all()
    assert irs.groups(4, 2).tolist() == [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3] and irs.groups(4, 2).dtype == np.uint16
    assert irs.groups(3, 1).tolist() == list(range(9)) and (irs.groups(6, 6) == 0).all()
    assert irs.est_scale(5) == np.float32(0.2) and irs.est_scale(5, 2.0, mmse=True) == np.float32(1 / 9)
    assert irs.est_scale(5, 2.0) == np.float32(0.2)
    for bad in (lambda: irs.groups(4, 3), lambda: irs.dft_pilots(0), lambda: irs.hadamard_pilots(1024), lambda: irs.est_scale(0)):
        with pytest.raises(ValueError):
            bad()


def test_mutation_table():
    """every check on the restatement and on every mutant: the check named for a mutant fails on it (the table that
    `pytest tests/test_irs_estimate_ref.py -k mutation_table -s` prints is kept as profiles/irs_estimate_mutations.txt)"""
    lines = ["mutant      " + "".join("%-26s" % f.__name__ for f in CHECKS.values())]
    for m in (None,) + er.MUTANTS:
        row = []
        for name, f in CHECKS.items():
            try:
                f(m)
                row.append("pass")
            except AssertionError:
                row.append("FAIL")
            if m is None or name == m:
                assert row[-1] == ("pass" if m is None else "FAIL"), (m, name)
        lines.append("%-12s" % (m or "(none)") + "".join("%-26s" % r for r in row))
    print("\n" + "\n".join(lines))
