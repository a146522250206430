"""NUMERICS.md rule 34 on the CPU: the generated table and its figures, the properties of the restatement tests/arb_ref.py
(1/1 hands its input back, a ratio is reduced first, cuts and shifts change no bit, the counting), its distance from the
float64 definition against the rule's derived bound, five mutants of the restatement each caught by the test named for it
(profiles/arb_mutations.txt), and the rule in front of the oracle's receiver: round trips through 25, 30.72, 40, 61.44 and
80 MS/s, and a victim channel between stronger neighbours taken out of an 80 MS/s capture."""
import importlib.util
import math
import os

import numpy as np
import pytest

import arb_ref as ar
import convert_ref as cr
from wifirx import capi, txgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [r for r in ar.RATIOS if r != (10, 8)]
RATIO_ID = ["%d_%d" % r for r in RATIOS]
OCC = 26.5 / 64


def _gen():
    spec = importlib.util.spec_from_file_location("gen_arb_table", os.path.join(ROOT, "tools", "gen_arb_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 2)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the table ---------------------------------------------------------------------------------------------------------

def test_header_is_the_generators_output():
    g = _gen()
    assert open(g.HEADER).read() == g.render()
    assert np.array_equal(bits(g.design()), bits(ar.table()))


def test_table_bounds():
    """rule 18's own bounds: 1e-3 of deviation from 1 over the occupied band (and with the 0.02 margin), -60 dB over all that
    folds onto it (and with the margin); the figures include the float32 rounding and the linear interpolation"""
    g = _gen()
    (p0, p1), (s0, s1) = g.figures(ar.table())
    print("passband %.3e / %.3e, stopband %.1f / %.1f dB" % (p0, p1, s0, s1))
    assert p0 <= 1e-3 and p1 <= 1e-3
    assert s0 <= -60.0 and s1 <= -60.0
    H = ar.table()
    assert H[16 * 128] == 1.0 and (H[::128][np.arange(33) != 16] == 0.0).all()
    assert np.array_equal(H, H[::-1])
    # 80 -> 20 MS/s: a tone at 11.7 MHz folds onto the occupied band and must be gone; one at 8 MHz passes
    assert g.tone_level_db(H, 4, 1, 11.7 / 80) <= -60.0
    assert abs(g.tone_level_db(H, 4, 1, 8.0 / 80)) <= 0.01


# ---- properties of the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("num,den", [(1, 1), (7, 7)])
def test_unit_ratio_returns_the_input(num, den):
    x = noise(500, 1)
    y = ar.resample(x, num, den)
    assert len(y) == 500 - 16
    assert np.array_equal(y, x[:len(y)])


def test_a_ratio_is_reduced_first():
    x = noise(700, 2)
    assert np.array_equal(bits(ar.resample(x, 10, 8)), bits(ar.resample(x, 5, 4)))
    assert ar.hist_len(10, 8) == ar.hist_len(5, 4) == 40 and ar.count(10, 8, 0, 700, 0) == ar.count(5, 4, 0, 700, 0)


@pytest.mark.parametrize("num,den", RATIOS, ids=RATIO_ID)
def test_count_is_the_brute_force_enumeration(num, den):
    """m_end(E): the outputs whose last input jhi(m) lies below E, for every E <= 300"""
    for E in range(0, 301):
        m = 0
        while ar.span(num, den, m)[1] < E:
            m += 1
        assert ar.m_end(num, den, E) == m == ar.count(num, den, 0, E, 0), E
    HL = ar.hist_len(num, den)
    S = max(num, den)
    assert HL == -((-32 * S) // den) <= ar.HIST_MAX
    # the output behind a call's last one starts inside the history that the call hands on
    for E in (1, HL, 257):
        assert ar.span(num, den, ar.m_end(num, den, E))[0] >= E - HL


@pytest.mark.parametrize("num,den", RATIOS, ids=RATIO_ID)
def test_a_stream_cut_into_calls_is_the_uncut_stream(num, den):
    HL = ar.hist_len(num, den)
    x = noise(900, 3 + num)
    whole = ar.resample(x, num, den)
    for cut in (1, HL, 257):
        a = ar.resample(x[:cut], num, den)
        hist = ar.next_history(x[:cut], None, num, den)
        b = ar.resample(x[cut:], num, den, hist, j0=cut, m0=len(a))
        assert np.array_equal(bits(np.concatenate([a, b])), bits(whole)), cut
    # and far into a stream: the same bytes with j0 near 2^50 when the pair (j0, m0) lies on the same phase
    k = (1 << 50) // num
    far = ar.resample(x[HL:], num, den, x[:HL], j0=HL + k * num, m0=k * den + ar.m_end(num, den, HL))
    near = ar.resample(x[HL:], num, den, x[:HL], j0=HL, m0=ar.m_end(num, den, HL))
    assert np.array_equal(bits(far), bits(near))


def test_integer_formats_are_widened_first():
    q = np.random.default_rng(4).integers(-128, 128, (300, 2)).astype(np.int8)
    got = ar.resample_format(q, cr.SC8, 2.0 ** -7, 5, 4)
    assert np.array_equal(bits(got), bits(ar.resample(cr.widen(q, 2.0 ** -7), 5, 4)))


def test_zeros_take_part_as_zeros():
    """a NULL history and a history of zeros give the same bytes"""
    x = noise(300, 5)
    for num, den in ((5, 4), (1, 2)):
        HL = ar.hist_len(num, den)
        m0 = ar.m_end(num, den, 1000)
        a = ar.resample(x, num, den, None, j0=1000, m0=m0)
        b = ar.resample(x, num, den, np.zeros((HL, 2), np.float32), j0=1000, m0=m0)
        assert len(a) and np.array_equal(bits(a), bits(b))


# ---- against the definition ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num,den", RATIOS, ids=RATIO_ID)
def test_restatement_against_the_definition(num, den):
    x = noise(1200, 10 * num + den)
    got = cr.to_complex(ar.resample(x, num, den)).astype(np.complex128)
    want = ar.direct(cr.to_complex(x), num, den)
    assert got.shape == want.shape
    bound = ar.error_bound(num, den, float(np.abs(x).max()))
    worst = max(float(np.abs(got.real - want.real).max()), float(np.abs(got.imag - want.imag).max()))
    print("%d/%d: worst |restatement - definition| per component = %.3e, bound %.3e" % (num, den, worst, bound))
    assert worst <= bound


# ---- the mutants: checks that take the restatement's `mutant` ----------------------------------------------------------------

def scalar_outputs(x, num, den, ms):
    """the rule read literally, one output and one float32 operation at a time (stream from j0 = m0 = 0)"""
    rn, rd = ar.reduce(num, den)
    gain = np.float32(rd) / np.float32(max(rn, rd))
    out = np.empty((len(ms), 2), np.float32)
    for i, m in enumerate(ms):
        jlo, c = ar.coefficients(num, den, m)
        acc = None
        for k in range(len(c)):
            j = jlo + k
            s = x[j] if j >= 0 else np.zeros(2, np.float32)
            t = np.array([c[k] * s[0], c[k] * s[1]], np.float32)
            acc = t if acc is None else acc + t
        out[i] = acc * gain if rn > rd else acc
    return out


def check_shifted_stream(mutant=None):
    """x behind num k zeros gives y behind den k outputs, bit for bit: the floors at negative numerators are floors"""
    for num, den in RATIOS:
        S = max(num, den)
        k = -((-16 * S) // (num * den)) + 1
        x = noise(400, 20 + num)
        y = ar.resample(x, num, den, mutant=mutant)
        ys = ar.resample(np.concatenate([np.zeros((num * k, 2), np.float32), x]), num, den, mutant=mutant)
        assert len(ys) == len(y) + den * k
        assert np.array_equal(ys[den * k:], y), (num, den)


def check_impulse_reads_out_the_coefficients(mutant=None):
    """impulses further apart than an output's taps: every output is the coefficient of the one impulse it reads (or zero),
    H[q] + frac (H[q+1] - H[q]) with frac = (float)r * (1 / S) -- some thousand (q, r) per ratio"""
    H = ar.table()
    # 96/125 and 125/96 (61.44 <-> 80 MS/s): S = 125 shares no factor with 128, so r takes every value below S
    for num, den in ((5, 4), (4, 5), (192, 125), (125, 192), (384, 125), (96, 125), (125, 96)):
        S = max(num, den)
        P = 32 * S // den + 2                                 # more than the most taps
        n = 6000
        x = np.zeros((n, 2), np.float32)
        x[P // 2::P] = (1.0, -1.0)
        y = ar.resample(x, num, den, mutant=mutant)
        m = np.arange(len(y), dtype=np.int64)
        jlo, jhi = (m * num - 16 * S) // den + 1, (m * num + 16 * S) // den
        j = -((-(jlo - P // 2)) // P) * P + P // 2            # the first impulse at or behind jlo
        reads = (j <= jhi) & (j >= 0)
        B = np.where(reads, (m * num - j * den + 16 * S) * 128, 0)
        q, r = B // S, B % S
        frac = r.astype(np.float32) * (np.float32(1) / np.float32(S))
        want = np.where(reads, H[q] + frac * (H[q + 1] - H[q]), np.float32(0))
        if num > den:
            want = want * (np.float32(den) / np.float32(S))
        assert want.dtype == np.float32 and reads.sum() > 1000
        assert np.array_equal(y[:, 0], want) and np.array_equal(y[:, 1], -want), (num, den)


def check_gain_is_one_multiply_behind_the_sum(mutant=None):
    for num, den in ((5, 4), (192, 125), (384, 125)):
        x = noise(700, 30 + num)
        ms = np.arange(60, 100)
        assert np.array_equal(bits(ar.resample(x, num, den, outputs=ms, mutant=mutant)), bits(scalar_outputs(x, num, den, ms))), (num, den)


def check_sum_runs_in_ascending_order(mutant=None):
    for num, den in ((4, 5), (1, 2), (125, 192), (1, 1)):
        x = noise(400, 40 + num)
        ms = np.concatenate([np.arange(0, 12), np.arange(200, 230)])
        assert np.array_equal(bits(ar.resample(x, num, den, outputs=ms, mutant=mutant)), bits(scalar_outputs(x, num, den, ms))), (num, den)


def check_every_output_reads_the_rules_taps(mutant=None):
    """an impulse at jlo(m) and at jhi(m) comes out of output m with the first and the last coefficient, one at jlo(m) - 1 or
    jhi(m) + 1 does not come out of it at all; the taps number floor(32 S / den) or one more"""
    seen = 0
    for num, den in RATIOS:
        S = max(num, den)
        gain = np.float32(den) / np.float32(S) if num > den else np.float32(1)
        for m in range(100, 112):
            jlo, jhi = ar.span(num, den, m)
            assert jhi - jlo + 1 in (32 * S // den, 32 * S // den + 1)
            _, c = ar.coefficients(num, den, m)
            for j, want in ((jlo - 1, np.float32(0)), (jlo, c[0]), (jhi, c[-1]), (jhi + 1, np.float32(0))):
                x = np.zeros((jhi + 40, 2), np.float32)
                x[j] = (1.0, 1.0)
                got = ar.resample(x, num, den, outputs=np.array([m]), mutant=mutant)[0, 0]
                assert got == (want * gain if num > den else want), (num, den, m, j)
                seen += int(want != 0)
    assert seen > 50                                          # the edge coefficients are not all zeros


CHECKS = {
    "test_a_shifted_stream_gives_the_shifted_output": check_shifted_stream,
    "test_an_impulse_reads_out_the_coefficients": check_impulse_reads_out_the_coefficients,
    "test_gain_is_one_multiply_behind_the_sum": check_gain_is_one_multiply_behind_the_sum,
    "test_sum_runs_in_ascending_order": check_sum_runs_in_ascending_order,
    "test_every_output_reads_the_rules_taps": check_every_output_reads_the_rules_taps,
}
NAMED = {
    "trunc_div": "test_a_shifted_stream_gives_the_shifted_output",
    "frac_div": "test_an_impulse_reads_out_the_coefficients",
    "gain_on_coef": "test_gain_is_one_multiply_behind_the_sum",
    "descending": "test_sum_runs_in_ascending_order",
    "jlo_off": "test_every_output_reads_the_rules_taps",
}


def test_a_shifted_stream_gives_the_shifted_output():
    check_shifted_stream()


def test_an_impulse_reads_out_the_coefficients():
    check_impulse_reads_out_the_coefficients()


def test_gain_is_one_multiply_behind_the_sum():
    check_gain_is_one_multiply_behind_the_sum()


def test_sum_runs_in_ascending_order():
    check_sum_runs_in_ascending_order()


def test_every_output_reads_the_rules_taps():
    check_every_output_reads_the_rules_taps()


def _fails(check, mutant):
    try:
        check(mutant)
    except AssertionError:
        return True
    return False


def mutation_table():
    names = list(CHECKS)
    rows = ["mutant        " + " ".join("T%d" % (i + 1) for i in range(len(names))) + "   named test"]
    caught = {}
    for mu in ar.MUTANTS:
        marks = ["x" if _fails(CHECKS[n], mu) else "." for n in names]
        caught[mu] = marks[names.index(NAMED[mu])] == "x"
        rows.append("%-13s " % mu + "  ".join(marks) + "    T%d" % (names.index(NAMED[mu]) + 1))
    legend = ["  T%d = %s" % (i + 1, n) for i, n in enumerate(names)]
    return "\n".join(legend + [""] + rows), caught


def test_every_mutant_is_caught_by_its_named_test():
    assert set(NAMED) == set(ar.MUTANTS)
    table, caught = mutation_table()
    print(table)
    assert all(caught.values()), caught
    txt = open(os.path.join(ROOT, "profiles", "arb_mutations.txt")).read()
    for mu in ar.MUTANTS:
        assert mu in txt and NAMED[mu] in txt


# ---- through the oracle ------------------------------------------------------------------------------------------------

ROUND_TRIPS = (((4, 5), (5, 4)), ((125, 192), (192, 125)), ((1, 2), (2, 1)), ((125, 384), (384, 125)), ((1, 4), (4, 1)))
SCENES = {"qpsk12": (2, 294, 12.0), "qam64_34": (7, 1000, 26.0)}
_scene_cache = {}


def scene(name):
    """32 frames behind a lead of 160 samples, a random CFO of +-0.03 rad/sample each, unit-variance noise: (stream, psdus, n_sym)"""
    if name not in _scene_cache:
        enc, plen, snr_db = SCENES[name]
        n_frames = 32
        psdu = txgen.make_psdus(n_frames, plen, seed=60 + enc)
        tx = txgen.encode_psdus(psdu, enc)
        cfo = np.random.default_rng(61 + enc).uniform(-0.03, 0.03, n_frames)
        total = 160 + tx.samples.shape[1] + 240
        # the noise seed is the first of 1, 2, .. with which the scene itself, without any resampling, decodes all 32
        x = txgen.impair(tx.samples, snr_db, cfo=cfo, lead=160, total=total, seed=1).reshape(-1)
        _scene_cache[name] = (x, psdu, tx.n_sym)
    return _scene_cache[name]


def decoded(x, n_sym, plen):
    """the PSDUs of the FCS-good frames of a stream, in order, through the oracle's receiver"""
    from oracle import oracle as orc
    prm = orc.make_params(max_sym=n_sym)
    o = orc.demod_stream(np.asarray(x, dtype=np.complex64), prm, cap=256)
    psdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
    ok = (o["frames"]["flags"] & capi.F_CRC_OK) != 0
    return psdu[ok][:, :plen]


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_decodes_without_the_round_trip(name):
    x, psdu, n_sym = scene(name)
    got = decoded(x, n_sym, psdu.shape[1])
    assert got.shape == psdu.shape and np.array_equal(got, psdu)


@pytest.mark.parametrize("up,down", ROUND_TRIPS, ids=["25", "30_72", "40", "61_44", "80"])
@pytest.mark.parametrize("name", list(SCENES))
def test_round_trip_in_front_of_the_oracle_receiver(name, up, down):
    """up to the capture rate and down again by the rule: every frame decodes to the transmitted PSDU, as without it"""
    x, psdu, n_sym = scene(name)
    n_up = len(x) * up[1] // up[0]
    wide = ar.stream(x, up[0], up[1], n_out=n_up)
    back = ar.stream(wide, down[0], down[1], n_out=len(x))
    got = decoded(back, n_sym, psdu.shape[1])
    lost = len(psdu) - sum(any(np.array_equal(g, p) for g in got) for p in psdu)
    print("%s through %d/%d then %d/%d: %d of %d lost" % (name, up[0], up[1], down[0], down[1], lost, len(psdu)))
    assert got.shape == psdu.shape and np.array_equal(got, psdu)


def adjacent_capture(db_up, n_frames=16, snr_db=28.0):
    """M = 4, stacking 0, the victim on stream 2 (the capture's centre), the other three `db_up` dB stronger and rolled by 800
    samples, unit-variance noise per channel bandwidth: (80 MS/s capture, the victim's PSDUs, n_sym)"""
    M, plen, enc = 4, 1000, 7
    streams, psdus, n_sym = [], None, 0
    for k in range(M):
        p = txgen.make_psdus(n_frames, plen, seed=70 + k)
        tx = txgen.encode_psdus(p, enc)
        row = np.zeros((n_frames, 160 + tx.samples.shape[1] + 240), np.complex128)
        row[:, 160:160 + tx.samples.shape[1]] = tx.samples
        v = row.reshape(-1)
        if k == 2:
            psdus, n_sym = p, tx.n_sym
        else:
            v = np.roll(v, 800)
        streams.append(v)
    gains = [math.sqrt(10 ** ((snr_db + (0.0 if k == 2 else db_up)) / 10)) for k in range(M)]
    wide = txgen.synthesise_wideband(streams, M, 0, gains)
    rng = np.random.default_rng(71)
    wide = wide + (rng.standard_normal(len(wide)) + 1j * rng.standard_normal(len(wide))) * math.sqrt(0.5 * M)
    return wide.astype(np.complex64), psdus, n_sym


def test_victim_between_stronger_neighbours():
    """the capture resampled 4/1: the victim's 16 frames decode with the neighbours 10 dB above it"""
    wide, psdus, n_sym = adjacent_capture(10.0)
    y = ar.stream(wide, 4, 1, n_out=len(wide) // 4)
    got = decoded(y, n_sym, psdus.shape[1])
    lost = len(psdus) - sum(any(np.array_equal(g, p) for g in got) for p in psdus)
    print("victim with neighbours +10 dB: %d of %d lost" % (lost, len(psdus)))
    assert lost == 0
