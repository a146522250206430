"""NUMERICS.md rule 25 on the host: tests/irs_ref.py (the NumPy float32 restatement of wifirx_irs_taps) and wifirx/irs.py
against the reference's own channel (tests/golden/irs_reference.npz, recorded by tools/make_golden_irs.py from
utils/SV_channel.py and utils/channel.py), the rule's clauses one by one, and the statistics of the Philox scatter."""
import math
import os

import numpy as np
import pytest

import irs_ref
from wifirx import irs

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "irs_reference.npz")
SCALES = (2, 4, 16)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def fixture_case(gold, S, u):
    tag = "S%d_u%d" % (S, u)
    return (gold["los_%s_b2r" % tag], gold["los_%s_r2u" % tag], gold["los_%s_b2u" % tag], gold["nlos_" + tag],
            gold["mix_" + tag], gold["psi_S%d" % S], gold["H_" + tag])


# ---- the reference's geometry and channel ----

@pytest.mark.parametrize("S", SCALES)
def test_los_equals_the_reference(gold, S):
    for u in range(2):
        b2r, r2u, b2u = irs.los(S, gold["irs_pos_S%d" % S], gold["ap_pos_S%d" % S], gold["user_pos_S%d" % S][u])
        want = fixture_case(gold, S, u)
        assert np.abs(b2r - want[0]).max() <= 1e-12 and np.abs(r2u - want[1]).max() <= 1e-12 and abs(b2u - want[2]) <= 1e-12


def test_fixture_mixes_are_the_mix_of_its_draws(gold):
    """the recorded mixes are the Rician mix of the recorded draws (the two calls share their seed), in float64"""
    k = float(gold["k_factor"])
    for S in SCALES:
        for u in range(2):
            b2r, r2u, b2u, nlos, mixes, psi, H = fixture_case(gold, S, u)
            los_row = np.concatenate([b2r, r2u, [b2u]])
            assert np.abs(math.sqrt(k / (k + 1)) * los_row + math.sqrt(1 / (k + 1)) * nlos - mixes).max() <= 1e-14
            N = S * S
            for j in range(2):
                h = (mixes[:, :N] * psi[j] * mixes[:, N:2 * N]).sum(axis=1) + mixes[:, 2 * N]
                assert np.abs(h - H[:, j]).max() <= 1e-12 * N


@pytest.mark.parametrize("S", SCALES)
def test_restatement_equals_the_reference_channel(gold, S):
    """given scatter = the reference's draws, K = 10, its psi: within rule 25's bound of getChnl's H"""
    worst = 0.0
    for u in range(2):
        b2r, r2u, b2u, nlos, mixes, psi, H = fixture_case(gold, S, u)
        N, n = S * S, nlos.shape[0]
        for j in range(2):
            got = irs_ref.irs_taps(n, [1.0], b2r, r2u, b2u, k_factor=float(gold["k_factor"]), psi=psi[j], scatter=nlos)
            lim = irs_ref.bound(mixes[:, 2 * N], mixes[:, :N], mixes[:, N:2 * N])
            err = np.abs(got["taps"][:, 0].astype(np.complex128) - H[:, j])
            worst = max(worst, float((err / lim).max()))
            assert (err <= lim).all(), (S, u, j, err / lim)
    print("S = %d: largest error / bound = %.3f" % (S, worst))


# ---- the clauses of the rule ----

def small(rng, N=70, L=3, n_sets=4, n_scatter=None):
    a, b, d = crandn(rng, N), crandn(rng, N), crandn(rng, 1)[0]
    psi = irs.random_psi(N, 3, 5)
    sc = crandn(rng, n_scatter or n_sets * L, 2 * N + 1)
    pdp = np.exp(-np.arange(L) / 2.0).astype(F32)
    return a, b, d, psi, sc, pdp


def test_rician_mix_limits():
    rng = np.random.default_rng(1)
    a, b, d, psi, sc, pdp = small(rng)
    N = a.size
    # k_factor = 0: the elements ARE the scatter, the line of sight is not looked at
    r0 = irs_ref.irs_taps(4, pdp, a, b, d, psi=psi, scatter=sc)
    nan = np.full(N, np.nan + 0j)
    rn = irs_ref.irs_taps(4, pdp, nan, nan, np.nan, psi=psi, scatter=sc)
    assert same(r0["taps"], rn["taps"])
    assert same(r0["elems"][:, :, 0, :], sc[:, :N].reshape(4, 3, N)) and same(r0["elems"][:, :, 1, :], sc[:, N:2 * N].reshape(4, 3, N))
    assert same(r0["direct"], sc[:, 2 * N].reshape(4, 3))
    # a K so large that a_los = 1 and a_nlos^2 underflows the sum: the elements are the line of sight
    rk = irs_ref.irs_taps(4, pdp, a, b, d, k_factor=1e30, psi=psi, scatter=sc)
    assert np.abs(rk["elems"][:, :, 0, :] - a).max() <= 1e-14 and np.abs(rk["elems"][:, :, 1, :] - b).max() <= 1e-14
    # K = 10: the coefficients are formed in double and rounded once
    co = irs_ref.rician(10.0)
    assert co[0] == F32(math.sqrt(10 / 11)) and co[1] == F32(math.sqrt(1 / 11))
    r10 = irs_ref.irs_taps(4, pdp, a, b, d, k_factor=10.0, psi=psi, scatter=sc)
    want = co[0] * a.real + co[1] * sc[0, :N].real
    assert same(r10["elems"][0, 0, 0, :].real, want)


def test_direct_gain_zero_blocks_the_direct_path():
    rng = np.random.default_rng(2)
    a, b, d, psi, sc, pdp = small(rng)
    r = irs_ref.irs_taps(4, pdp, a, b, None, k_factor=3.0, direct_gain=0.0, psi=psi, scatter=sc)
    assert same(r["direct"], np.zeros((4, 3), np.complex64))
    sc2 = sc.copy()
    sc2[:, -1] = 1e9
    assert same(irs_ref.irs_taps(4, pdp, a, b, 7.0, k_factor=3.0, direct_gain=0.0, psi=psi, scatter=sc2)["taps"], r["taps"])
    # and it is one multiply per part otherwise
    half = irs_ref.irs_taps(4, pdp, a, b, d, k_factor=3.0, direct_gain=0.5, psi=psi, scatter=sc)
    one = irs_ref.irs_taps(4, pdp, a, b, d, k_factor=3.0, direct_gain=1.0, psi=psi, scatter=sc)
    assert same(half["direct"], (one["direct"] * F32(0.5)).astype(np.complex64))


def test_psi_sets_and_scatter_rows_wrap():
    rng = np.random.default_rng(3)
    a, b, d, psi, sc, pdp = small(rng, n_sets=5, n_scatter=7)
    N, L = a.size, pdp.size
    psis = np.stack([psi, irs.random_psi(N, 2, 6)])
    r = irs_ref.irs_taps(5, pdp, a, b, d, k_factor=2.0, psi=psis, scatter=sc)
    for s in range(5):
        for l in range(L):
            alone = irs_ref.irs_taps(1, pdp[l:l + 1], a, b, d, k_factor=2.0, psi=psis[s % 2], scatter=sc[(s * L + l) % 7][None])
            assert same(alone["taps"][0, 0], r["taps"][s, l]), (s, l)


def test_sum_order_is_the_waves():
    """a case where the order shows: the lane / butterfly sum differs from the plain ascending sum, and is restated alone"""
    rng = np.random.default_rng(4)
    p = (rng.standard_normal((3, 130)) * 10.0 ** rng.integers(-3, 4, (3, 130))).astype(F32)
    got = irs_ref.wave_sum(p)
    for i in range(3):
        lanes = [F32(0)] * 64
        for n in range(130):
            lanes[n % 64] = p[i, n] if n < 64 else F32(lanes[n % 64] + p[i, n])
        for m in (32, 16, 8, 4, 2, 1):
            lanes = [F32(lanes[k] + lanes[k ^ m]) for k in range(64)]
        assert lanes[0] == got[i]
    plain = np.array([np.add.accumulate(p[i])[-1] for i in range(3)])
    assert (plain != got).any()
    one = irs_ref.wave_sum(np.array([[F32(-0.0)]]))
    assert np.signbit(one[0]) == False                      # -0 + the empty lanes' +0


def test_tie_rule_lowest_code_wins():
    # e on the real axis, direct path blocked: C_0 wins alone; e = 0: every metric ties at 0, code 0; e exactly between
    # C_0 and C_1 of a 2-bit surface (45 degrees): both metrics are equal, the lower code stays
    er = np.array([1.0, 0.0, 1.0, -1.0, 1.0], F32)
    ei = np.array([0.0, 0.0, -1.0, -1.0, 1.0], F32)
    codes = irs.align_codes(er, ei, 0.0, 0.0, 2)
    # Re(e C_c) for c = 0..3: e = 1-1j -> (1, 1, -1, -1): tie of 0 and 1 -> 0; e = -1-1j -> (-1, 1, 1, -1): tie of 1 and 2 -> 1;
    # e = 1+1j -> (1, -1, -1, 1): tie of 0 and 3 -> 0
    assert codes.tolist() == [0, 0, 0, 1, 0]
    # with a direct path the target is its direction: d = j, e = 1 -> psi = j (code 1 of 2 bits)
    assert irs.align_codes(np.array([1.0], F32), np.array([0.0], F32), 0.0, 1.0, 2).tolist() == [1]


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_align_equals_the_genie_without_scatter(bits):
    """zero scatter and a K so large that a_los = 1: the genie's codes are the geometry's"""
    b2r, r2u, b2u = irs.los(6, [0.015, 0.015, 0], [0.09, 0.09, 4.5], [0.39, -0.11, 1.0])
    N = 36
    codes, psi = irs.align(b2r, r2u, b2u, bits)
    r = irs_ref.irs_taps(2, [1.0, 0.5], b2r, r2u, b2u, k_factor=1e30, align_bits=bits, scatter=np.zeros((1, 2 * N + 1), np.complex64))
    assert np.array_equal(r["codes"], np.stack([codes, codes]))
    fixed = irs_ref.irs_taps(2, [1.0, 0.5], b2r, r2u, b2u, k_factor=1e30, psi=psi, scatter=np.zeros((1, 2 * N + 1), np.complex64))
    assert same(fixed["taps"], r["taps"])
    # the aligned surface adds in phase with the direct path: within the quantisation loss of N + 1
    assert abs(r["taps"][0, 0]) >= 1 + N * math.cos(math.pi / (1 << bits)) - 1e-3
    assert codes.max() < (1 << bits) and psi.dtype == np.complex64


def test_genie_decides_on_tap_zero_for_every_tap():
    rng = np.random.default_rng(8)
    a, b, d, psi, sc, pdp = small(rng, N=65, L=3, n_sets=2)
    r3 = irs_ref.irs_taps(2, pdp, a, b, d, k_factor=1.0, align_bits=2, scatter=sc)
    # tap 0 alone of each set (its scatter row: (r L + 0) % n_scatter) gives the same codes
    for s in range(2):
        r1 = irs_ref.irs_taps(1, pdp[:1], a, b, d, k_factor=1.0, align_bits=2, scatter=sc[3 * s][None])
        assert np.array_equal(r1["codes"][0], r3["codes"][s])
    # and the other taps use them: the taps equal the given-psi call with those phases
    for s in range(2):
        fixed = irs_ref.irs_taps(2, pdp, a, b, d, k_factor=1.0, psi=irs.PHASES[r3["codes"][s].astype(int) << 1], scatter=sc)
        assert same(fixed["taps"][s], r3["taps"][s])


def test_tap_scale_is_formed_in_double():
    rng = np.random.default_rng(9)
    a, b, d, psi, sc, pdp = small(rng, L=2, n_sets=1)
    pdp = np.array([0.3, 0.07], F32)
    one = irs_ref.irs_taps(1, [1.0, 1.0], a, b, d, psi=psi, scatter=sc)["taps"]
    got = irs_ref.irs_taps(1, pdp, a, b, d, gain=1.7, psi=psi, scatter=sc)["taps"]
    for l in range(2):
        s = F32(math.sqrt(float(pdp[l])) * float(F32(1.7)))
        assert got[0, l].real == one[0, l].real * s and got[0, l].imag == one[0, l].imag * s


# ---- the statistics of the Philox scatter ----

SETS = 4096


@pytest.mark.parametrize("N", [16, 64, 256])
def test_random_phases_give_n_plus_one(N):
    """K = 0, L = 1, pdp = {1}: N + 1 independent unit-power terms; five standard errors of the mean are at most 8.4 %"""
    one = np.ones(N, np.complex64)
    t = irs_ref.irs_taps(SETS, [1.0], one, one, 1.0, psi=irs.random_psi(N, 2, N), seed=0xC0FFEE + N)["taps"][:, 0]
    mean = float((np.abs(t.astype(np.complex128)) ** 2).mean())
    print("N = %d: mean |t|^2 = %.2f (N + 1 = %d)" % (N, mean, N + 1))
    assert abs(mean - (N + 1)) <= 0.10 * (N + 1)


@pytest.mark.parametrize("N,bits", [(64, 1), (64, 2), (64, 3), (16, 2)])
def test_aligned_phases_reach_the_quantised_array_gain(N, bits):
    """E|ab| = pi/4 and a residual phase uniform within +-pi/2^B: by Jensen E|t|^2 >= (N pi/4 sinc(pi/2^B))^2"""
    one = np.ones(N, np.complex64)
    t = irs_ref.irs_taps(SETS, [1.0], one, one, 1.0, align_bits=bits, seed=77 + bits)["taps"][:, 0]
    mean = float((np.abs(t.astype(np.complex128)) ** 2).mean())
    x = math.pi / (1 << bits)
    floor = (N * math.pi / 4 * math.sin(x) / x) ** 2
    print("N = %d, B = %d: mean |t|^2 = %.1f, bound %.1f" % (N, bits, mean, floor))
    assert mean >= 0.9 * floor


def test_draws_depend_on_seed_set_and_tap():
    wa, wb, wd = irs_ref.draws(2, 2, 8, 5)
    wa2, _, wd2 = irs_ref.draws(2, 2, 8, 6)
    assert not same(wa, wa2) and not same(wd, wd2)
    flat = np.concatenate([wa.reshape(-1), wb.reshape(-1), wd.reshape(-1)])
    assert np.unique(flat).size == flat.size
