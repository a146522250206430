"""NUMERICS.md rules 27 and 28 on the host: tests/irs_multi_ref.py against the reference's own multi-antenna channel
(tests/golden/irs_multi_reference.npz, recorded by tools/make_golden_irs_multi.py from utils/SV_channel.py with antennaNum = 2 and 4),
against the single-antenna restatements (tests/irs_ref.py, tests/irs_sweep_ref.py), and clause by clause."""
import math
import os

import numpy as np
import pytest

import irs_multi_ref as mr
import irs_ref
import irs_sweep_ref as sr
from wifirx import irs

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "irs_multi_reference.npz")
CASES = [(S, M) for S in (2, 4) for M in (2, 4)]


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def small(rng, M=3, N=70, L=3, n_sets=4):
    pdp = np.exp(-np.arange(L) / 2.0).astype(F32)
    return crandn(rng, M, N), crandn(rng, N), crandn(rng, M), pdp, crandn(rng, n_sets * L - 1, (M + 1) * N + M)


# ---- the reference's geometry and channel ----

@pytest.mark.parametrize("S,M", CASES)
def test_los_equals_the_reference(gold, S, M):
    tag = "S%d_M%d" % (S, M)
    pos = [gold["%s_pos_S%d" % (k, S)] for k in ("irs", "ap", "user")]
    b2r, r2u, b2u = irs.los(S, *pos, antennas=M)
    assert b2r.shape == (M, S * S) and r2u.shape == (S * S,) and b2u.shape == (M,)
    assert np.abs(b2r - gold["los_%s_b2r" % tag]).max() <= 1e-12 and np.abs(r2u - gold["los_%s_r2u" % tag]).max() <= 1e-12
    assert np.abs(b2u - gold["los_%s_b2u" % tag]).max() <= 1e-12
    # the default is what it was, and antenna 0 of the array is it
    one = irs.los(S, *pos)
    assert one[0].shape == (S * S,) and one[2] == complex(1.0) and np.array_equal(one[0], b2r[0]) and np.array_equal(one[1], r2u)
    with pytest.raises(ValueError):
        irs.los(S, *pos, antennas=9)
    with pytest.raises(ValueError):
        irs.los(S, *pos, antennas=0)


@pytest.mark.parametrize("S,M", CASES)
def test_restatement_equals_the_reference_channel(gold, S, M):
    """given scatter = the reference's draws, K = 10, its psi: within rule 25's bound of getChnl's H, per antenna"""
    tag, N = "S%d_M%d" % (S, M), S * S
    nlos, mixes, psi, H = gold["nlos_" + tag], gold["mix_" + tag], gold["psi_S%d" % S], gold["H_" + tag]
    k = float(gold["k_factor"])
    los_row = np.concatenate([gold["los_%s_b2r" % tag].reshape(-1), gold["los_%s_r2u" % tag], gold["los_%s_b2u" % tag]])
    assert np.abs(math.sqrt(k / (k + 1)) * los_row + math.sqrt(1 / (k + 1)) * nlos - mixes).max() <= 1e-14
    n, worst = nlos.shape[0], 0.0
    for j in range(2):
        got = mr.irs_taps_multi(n, [1.0], gold["los_%s_b2r" % tag], gold["los_%s_r2u" % tag], gold["los_%s_b2u" % tag], k_factor=k,
                                psi=psi[j], scatter=nlos)
        for m in range(M):
            lim = irs_ref.bound(mixes[:, (M + 1) * N + m], mixes[:, m * N:(m + 1) * N], mixes[:, M * N:(M + 1) * N])
            err = np.abs(got["taps"][m, :, 0].astype(np.complex128) - H[:, j, m])
            worst = max(worst, float((err / lim).max()))
            assert (err <= lim).all(), (S, M, j, m, err / lim)
    print("S = %d, M = %d: largest error / bound = %.3f" % (S, M, worst))


# ---- against the single-antenna rules ----

def test_one_antenna_is_rules_25_and_26():
    rng = np.random.default_rng(1)
    a, b, d, pdp, sc = small(rng, M=1)
    cb = np.exp(1j * rng.uniform(-np.pi, np.pi, (17, 70))).astype(np.complex64)
    for src in (dict(scatter=sc), dict(seed=0x123456789)):
        for ph in (dict(psi=irs.random_psi(70, 3, 5)), dict(align_bits=2)):
            kw = dict(k_factor=3.0, gain=0.7, **src, **ph)
            got, want = mr.irs_taps_multi(4, pdp, a, b, d, **kw), irs_ref.irs_taps(4, pdp, a[0], b, d[0], **kw)
            assert same(got["taps"][0], want["taps"]) and same(got["elems"], want["elems"]) and same(got["direct"][0], want["direct"])
            assert (got["codes"] is None) == (want["codes"] is None) and (got["codes"] is None or np.array_equal(got["codes"], want["codes"]))
        got = mr.irs_sweep_multi(4, pdp, a, b, d, codebook=cb, k_factor=3.0, **src)
        want = sr.irs_sweep(4, pdp, a[0], b, d[0], codebook=cb, k_factor=3.0, **src)
        assert same(got["power"], want["power"]) and np.array_equal(got["best"], want["best"]) and same(got["taps"][0], want["taps"])


@pytest.mark.parametrize("M", [2, 5, 8])
def test_antenna_zero_is_the_single_antenna_call(M):
    rng = np.random.default_rng(M)
    a, b, d, pdp, sc = small(rng, M=M)
    for ph in (dict(psi=crandn(rng, 2, 70)), dict(align_bits=1), dict(align_bits=3)):
        kw = dict(k_factor=10.0, seed=77, **ph)                    # Philox: antenna 0's counters are rule 25's
        got, want = mr.irs_taps_multi(4, pdp, a, b, d, **kw), irs_ref.irs_taps(4, pdp, a[0], b, d[0], **kw)
        assert same(got["taps"][0], want["taps"]) and same(got["elems"][:, :, 0], want["elems"][:, :, 0])
        assert same(got["elems"][:, :, M], want["elems"][:, :, 1])
        if "align_bits" in ph:                                     # the genie of the reference antenna: its codes, for everyone
            assert np.array_equal(got["codes"], want["codes"])
            psi = irs.PHASES[got["codes"].astype(np.intp) << (3 - ph["align_bits"])]
            assert same(got["taps"], mr.irs_taps_multi(4, pdp, a, b, d, k_factor=10.0, seed=77, psi=psi)["taps"])
        kw = dict(k_factor=10.0, scatter=sc, **ph)                 # given scatter: the rows (w_a[0], w_b, w_d[0])
        got = mr.irs_taps_multi(4, pdp, a, b, d, **kw)
        want = irs_ref.irs_taps(4, pdp, a[0], b, d[0], **dict(kw, scatter=mr.antenna_rows(sc, M, 70, 0)))
        assert same(got["taps"][0], want["taps"])


def test_every_antenna_shares_the_surface_to_user_leg():
    rng = np.random.default_rng(3)
    a, b, d, pdp, sc = small(rng, M=4)
    for src in (dict(scatter=sc), dict(seed=5)):
        got = mr.irs_taps_multi(4, pdp, a, b, d, k_factor=2.0, psi=np.ones(70), **src)
        for m in range(4):
            one = irs_ref.irs_taps(4, pdp, a[m], b, d[m], k_factor=2.0, psi=np.ones(70),
                                   scatter=mr.antenna_rows(mr.given(4, 3, 70, 4, src.get("scatter"), src.get("seed", 0)), 4, 70, m))
            assert same(got["taps"][m], one["taps"]) and same(one["elems"][:, :, 1], got["elems"][:, :, 4])
        if "seed" in src:                                          # (the given rows wrap: 11 rows for 12 pairs)
            assert np.unique(got["elems"][:, :, :4]).size == 4 * 4 * 3 * 70


# ---- rule 28's metric ----

def test_power_is_summed_in_ascending_rho():
    rng = np.random.default_rng(4)
    M, L, N, K, n_sets = 3, 6, 33, 9, 3
    a, b, d, pdp, sc = small(rng, M=M, N=N, L=L, n_sets=n_sets)
    cb = np.exp(1j * rng.uniform(-np.pi, np.pi, (K, N))).astype(np.complex64)
    got = mr.irs_sweep_multi(n_sets, pdp, a, b, d, codebook=cb, k_factor=3.0, scatter=sc)
    t = got["all_taps"]
    order_matters = False
    for r in range(n_sets):
        for k in range(K):
            p, rev = None, F32(0)
            for m in range(M):                                     # rho = m L + l ascending, from q_0
                for l in range(L):
                    re, im = F32(t[m, r, l, k].real), F32(t[m, r, l, k].imag)
                    q = F32(F32(re * re) + F32(im * im))
                    p = q if p is None else F32(p + q)
            for l in range(L):                                     # another order: l outermost
                for m in range(M):
                    rev = F32(rev + F32(F32(t[m, r, l, k].real) ** 2 + F32(t[m, r, l, k].imag) ** 2))
            assert p.view(np.uint32) == got["power"][r, k].view(np.uint32)
            order_matters |= bool(rev != p)
    assert order_matters                                           # the order is part of the rule: another one rounds differently
    # the winner's taps are the entry's, for every antenna
    for r in range(n_sets):
        assert same(got["taps"][:, r], t[:, r, :, got["best"][r]])
    # one tap: the sum over the antennas of rule 26's powers
    one = mr.irs_sweep_multi(n_sets, pdp[:1], a, b, d, codebook=cb, k_factor=3.0, scatter=sc[:, :])
    singles = [sr.irs_sweep(n_sets, pdp[:1], a[m], b, d[m], codebook=cb, k_factor=3.0, scatter=mr.antenna_rows(sc, M, N, m))["power"]
               for m in range(M)]
    assert same(one["power"], (singles[0] + singles[1]) + singles[2])


def test_tie_rule_and_nan():
    rng = np.random.default_rng(5)
    a, b, d, pdp, sc = small(rng, M=2, N=20, L=2)
    two = np.exp(1j * rng.uniform(-np.pi, np.pi, (2, 20))).astype(np.complex64)
    kw = dict(k_factor=3.0, scatter=sc)
    got = mr.irs_sweep_multi(4, pdp, a, b, d, codebook=np.stack([two[0], two[1], two[1], two[0]]), **kw)
    assert same(got["power"][:, 0], got["power"][:, 3]) and (got["best"] < 2).all()          # the lowest k wins a tie
    for at in (0, 2):
        cb = np.stack([two[0], two[1], two[0]])
        cb[at, 7] = np.nan
        got = mr.irs_sweep_multi(4, pdp, a, b, d, codebook=cb, **kw)
        assert np.isnan(got["power"][:, at]).all() and (got["best"] != at).all()             # a NaN never wins
    cb = np.stack([two[0], two[1]])
    cb[:, 3] = np.nan
    assert (mr.irs_sweep_multi(4, pdp, a, b, d, codebook=cb, **kw)["best"] == 0).all()       # all NaN: entry 0
    # a NaN on one antenna alone spoils the sum: the metric is the sum, not the best antenna
    a2 = a.copy()
    a2[1, 0] = np.nan
    assert np.isnan(mr.irs_sweep_multi(4, pdp, a2, b, d, codebook=two, **kw)["power"]).all()


# ---- the Philox assignment ----

def test_counters_of_the_antennas_are_distinct():
    """(counter word 2, word pair) per antenna and tap: none is rule 25's, none is used twice, one draw serves two antennas"""
    used = {}
    for l in range(16):
        used[(l, (0, 1))] = "a0"                                   # rule 25's w_a and w_d(0) ...
        used[(l, (2, 3))] = "b"                                    # ... and w_b (the direct path's (z, w) are not used)
    for m in range(1, 8):
        for l in range(16):
            key = (mr.counter_l(l, m), mr.words(m))
            assert key[0] >= 16 and key not in used, (m, l)        # l < 16: never rule 25's counters
            used[key] = "a%d" % m
    assert mr.counter_l(5, 0) == 5 and mr.words(0) == (0, 1)
    for j in range(1, 4):                                          # antennas 2 j - 1 and 2 j share a counter, on different words
        assert mr.counter_l(3, 2 * j - 1) == mr.counter_l(3, 2 * j) == 3 + 16 * j
        assert mr.words(2 * j - 1) == (0, 1) and mr.words(2 * j) == (2, 3)
    assert mr.counter_l(3, 7) == 3 + 64 and mr.words(7) == (0, 1)
    assert len({mr.counter_l(l, m) for m in (0, 1, 3, 5, 7) for l in range(16)}) == 80
    # and the draws themselves: every (antenna, r, l, n), the shared leg and the direct paths are values of their own
    wa, wb, wd = mr.draws(3, 16, 5, 8, seed=9)
    assert wa.shape == (8, 3, 16, 5) and wb.shape == (3, 16, 5) and wd.shape == (8, 3, 16)
    every = np.concatenate([wa.reshape(-1), wb.reshape(-1), wd.reshape(-1)])
    assert np.unique(every).size == every.size
    wa0, wb0, wd0 = irs_ref.draws(3, 16, 5, seed=9)
    assert same(wa[0], wa0) and same(wb, wb0) and same(wd[0], wd0)


def test_scatter_legs_are_independent():
    """sample correlations over one fixed seed, 4096 sets of 16 elements: the antenna pairs (0, 1), (1, 2), (2, 3) -- (1, 2)
    share a Philox call, (0, 1) and (2, 3) straddle two -- and every antenna against the shared leg stay below 5 / sqrt(n)"""
    wa, wb, _ = mr.draws(4096, 1, 16, 4, seed=2027)
    n = wb.size
    lim = 5.0 / math.sqrt(n)

    def rho(x, y):
        x, y = x.reshape(-1).astype(np.complex128), y.reshape(-1).astype(np.complex128)
        return abs(np.vdot(x - x.mean(), y - y.mean())) / (n * x.std() * y.std())

    got = {"a%d,a%d" % p: rho(wa[p[0]], wa[p[1]]) for p in ((0, 1), (1, 2), (2, 3))}
    got.update({"a%d,b" % m: rho(wa[m], wb) for m in range(4)})
    print("sample correlations (limit %.4f): %s" % (lim, ", ".join("%s %.4f" % kv for kv in got.items())))
    assert max(got.values()) < lim, got
    assert abs(float((np.abs(wa) ** 2).mean()) - 1.0) < 0.02
