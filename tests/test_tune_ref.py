"""NUMERICS.md rule 35 on the CPU: the properties of the restatement tests/tune_ref.py (a channel at the capture's centre is
rule 34 untouched, the increments, cuts change no bit, a NULL history is a history of zeros), its distance from the float64
definition against the rule's derived bound, a tone at its place, five mutants of the restatement each caught by the test
named for it (profiles/tune_mutations.txt), and the rule in front of the oracle's receiver: channels 1 / 6 / 11 out of one
80 MS/s capture."""
import os

import numpy as np
import pytest

import arb_ref as ar
import convert_ref as cr
import tune_ref as tr
from oracle import oracle as orc
from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [(4, 1), (5, 4), (384, 125), (1, 1)]
RATIO_ID = ["%d_%d" % r for r in RATIOS]
M64 = tr.M64
INC_25 = 0xB000000000000000                                   # +25 MHz in 80 MS/s: -5/16 turn per sample
PH = 0x3243F6A8885A308D                                       # a phase0 with every bit in use


def noise(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 2)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- properties --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num,den", RATIOS, ids=RATIO_ID)
def test_a_zero_channel_is_rule_34_bit_for_bit(num, den):
    x = noise(700, 1)
    x[100, 0], x[300, 1] = np.nan, np.inf
    HL = ar.hist_len(num, den)
    h = noise(HL, 2)
    j0 = 5000
    m0 = ar.m_end(num, den, j0)
    got = tr.tune(x, num, den, [INC_25, 0, 1], [PH, 0, 0], h, j0, m0)
    want = ar.resample(x, num, den, h, j0, m0)
    assert got.shape == (3,) + want.shape
    assert np.array_equal(bits(got[1]), bits(want))
    assert not np.array_equal(bits(got[0]), bits(want)) and not np.array_equal(bits(got[2]), bits(want))
    # a phase0 alone rotates
    assert not np.array_equal(bits(tr.tune(x, num, den, [0], [1 << 62], h, j0, m0)[0]), bits(want))


def test_tune_inc_values():
    assert tr.tune_inc(25e6, 80e6) == INC_25
    assert tr.tune_inc(-25e6, 80e6) == 0x5000000000000000
    assert tr.tune_inc(0.0, 80e6) == 0
    assert tr.tune_inc(40e6, 80e6) == tr.tune_inc(-40e6, 80e6) == 1 << 63
    assert tr.tune_inc(80e6 + 25e6, 80e6) == INC_25           # whole turns drop out
    rng = np.random.default_rng(3)
    for off in rng.uniform(-40e6, 40e6, 200):
        assert (tr.tune_inc(off, 80e6) + tr.tune_inc(-off, 80e6)) & M64 == 0, off
    # the increment brings the channel DOWN: a tone at +offset, rotated by it, stands still
    inc = tr.tune_inc(10e6, 80e6)
    j = np.arange(64)
    tone = np.exp(2j * np.pi * j / 8.0)
    ramp = np.exp(2j * np.pi * np.array([((inc * int(v)) & M64) / 2.0 ** 64 for v in j]))
    assert np.abs(tone * ramp - 1.0).max() < 1e-12


def check_every_sample_is_rotated_at_its_own_stream_index(mutant=None):
    """an impulse at stream index j comes out of every output that reads it as (coefficient) * (the phasor of j), whatever
    the output's own instant: the rotation stands in front of the sum"""
    num, den, j0 = 4, 1, 4096
    HL = ar.hist_len(num, den)
    m0 = ar.m_end(num, den, j0)
    x = np.zeros((600, 2), np.float32)
    at = 333
    x[at] = (1.0, 0.0)
    got = tr.tune(x, num, den, [INC_25 + 12345], [PH], np.zeros((HL, 2), np.float32), j0, m0, mutant=mutant)[0]
    plain = ar.resample(x, num, den, None, j0, m0)
    one = tr.rotate(np.array([[1.0, 0.0]], np.float32), INC_25 + 12345, PH, j0 + at)[0]
    hit = plain[:, 0] != 0
    assert hit.sum() > 20
    gain = np.float32(den) / np.float32(max(num, den))
    coef = plain[:, 0] / gain                                 # exact: the gain is a power of two at 4/1
    assert np.array_equal(got[hit, 0], (coef * one[0] * gain)[hit]) and np.array_equal(got[hit, 1], (coef * one[1] * gain)[hit])


def test_every_sample_is_rotated_at_its_own_stream_index():
    check_every_sample_is_rotated_at_its_own_stream_index()


def check_cuts(mutant=None):
    for num, den in RATIOS:
        HL = ar.hist_len(num, den)
        x = noise(900, 3 + num)
        incs, phs = [INC_25, 0, 0x1234567890ABCDEF], [0, 0, PH]
        whole = tr.tune(x, num, den, incs, phs, mutant=mutant)
        for cut in (1, HL, 257):
            a = tr.tune(x[:cut], num, den, incs, phs, mutant=mutant)
            hist = ar.next_history(x[:cut], None, num, den)   # raw samples, as rule 34 hands them on
            b = tr.tune(x[cut:], num, den, incs, phs, hist, j0=cut, m0=a.shape[1], mutant=mutant)
            assert np.array_equal(bits(np.concatenate([a, b], axis=1)), bits(whole)), (num, den, cut)
        # far into a stream: the same bytes as near its start when (j0, m0) lie on the same phase of the ratio and phase0
        # makes up for the 2^50 samples in between
        k = (1 << 50) // num
        near = tr.tune(x[HL:], num, den, incs, phs, x[:HL], j0=HL, m0=ar.m_end(num, den, HL), mutant=mutant)
        far = tr.tune(x[HL:], num, den, incs, [(p - i * k * num) & M64 for i, p in zip(incs, phs)], x[:HL], j0=HL + k * num,
                      m0=k * den + ar.m_end(num, den, HL), mutant=mutant)
        assert np.array_equal(bits(far), bits(near)), (num, den)
        # and it is cut there like anywhere else
        j0 = HL + k * num
        m0 = k * den + ar.m_end(num, den, HL)
        whole = tr.tune(x[HL:], num, den, incs, phs, x[:HL], j0=j0, m0=m0, mutant=mutant)
        a = tr.tune(x[HL:HL + 257], num, den, incs, phs, x[:HL], j0=j0, m0=m0, mutant=mutant)
        b = tr.tune(x[HL + 257:], num, den, incs, phs, ar.next_history(x[HL:HL + 257], x[:HL], num, den), j0=j0 + 257,
                    m0=m0 + a.shape[1], mutant=mutant)
        assert np.array_equal(bits(np.concatenate([a, b], axis=1)), bits(whole)), (num, den, "far")


def test_a_stream_cut_into_calls_is_the_uncut_stream():
    check_cuts()


def check_null_history(mutant=None):
    """a NULL history and a history of zeros give the same bytes.  The rotated zeros differ from plain ones only in their
    sign bits, and a sign survives a sum only where every term is a zero: 1/1, whose coefficients beside the centre are
    exact zeros, on a stretch of zero samples, with the phase in the second quadrant (cos < 0 < sin: 0 cs - 0 sn = -0)"""
    for num, den in ((5, 4), (1, 2), (4, 1)):
        HL = ar.hist_len(num, den)
        x = noise(300, 5)
        m0 = ar.m_end(num, den, 1000)
        a = tr.tune(x, num, den, [INC_25], [PH], None, j0=1000, m0=m0, mutant=mutant)
        b = tr.tune(x, num, den, [INC_25], [PH], np.zeros((HL, 2), np.float32), j0=1000, m0=m0, mutant=mutant)
        assert a.shape[1] and np.array_equal(bits(a), bits(b))
    x = noise(100, 6)
    x[:40] = 0
    inc, ph = 1 << 40, 3 << 61                                # 3/8 turn, all but standing still
    m0 = ar.m_end(1, 1, 1000)
    a = tr.tune(x, 1, 1, [inc], [ph], None, j0=1000, m0=m0, mutant=mutant)
    b = tr.tune(x, 1, 1, [inc], [ph], np.zeros((32, 2), np.float32), j0=1000, m0=m0, mutant=mutant)
    assert np.signbit(b[0, :8, 0]).all() and not np.signbit(b[0, :8, 1]).any()      # (-0, +0): the zeros were rotated
    assert np.array_equal(bits(a), bits(b))
    # and the zeros in front of a stream are rotated like any others
    c = tr.tune(x, 1, 1, [inc], [ph], mutant=mutant)
    assert np.signbit(c[0, :8, 0]).all() and not np.signbit(c[0, :8, 1]).any()


def test_a_null_history_is_a_history_of_zeros():
    check_null_history()


# ---- against the definition ----------------------------------------------------------------------------------------------

def check_against_the_definition(mutant=None):
    for num, den in RATIOS:
        x = noise(1200, 10 * num + den)
        for inc, ph in ((INC_25, PH), (0x5000000000000000, 0), (0x0123456789ABCDEF, 1 << 63)):
            got = cr.to_complex(tr.tune(x, num, den, [inc], [ph], mutant=mutant)[0]).astype(np.complex128)
            want = tr.direct(cr.to_complex(x), num, den, inc, ph)
            assert got.shape == want.shape
            bound = tr.error_bound(num, den, float(np.abs(x).max()))
            worst = max(float(np.abs(got.real - want.real).max()), float(np.abs(got.imag - want.imag).max()))
            if mutant is None:
                print("%d/%d inc %016x: worst |restatement - definition| per component = %.3e, bound %.3e" % (num, den, inc, worst, bound))
            assert worst <= bound, (num, den, inc)


def test_restatement_against_the_definition():
    check_against_the_definition()


def check_tone(mutant=None):
    """a tone 1 MHz above a channel at +25 MHz in 80 MS/s comes out of that channel at 1 MHz of 20 MS/s with rule 34's
    passband deviation (1e-3), and with the phase of the definition; the channel at -25 MHz holds none of it (-60 dB)"""
    n = 4000
    j = np.arange(n)
    x = np.exp(2j * np.pi * ((j * 26) % 80) / 80.0).astype(np.complex64)
    y = tr.stream(x, 4, 1, [INC_25, 0x5000000000000000], mutant=mutant)
    m = np.arange(40, y.shape[1] - 40)
    want = np.exp(2j * np.pi * ((m * 1) % 20) / 20.0)
    err = float(np.abs(y[0, m] - want).max())
    leak = float(np.abs(y[1, m]).max())
    if mutant is None:
        print("tone at offset + 1 MHz: |y - exp(j 2 pi m / 20)| <= %.2e, other channel %.1f dB" % (err, 20 * np.log10(leak)))
    assert err <= 1e-3
    assert leak <= 1e-3


def test_a_tone_comes_out_at_its_offset_from_the_tuned_centre():
    check_tone()


# ---- the mutants ------------------------------------------------------------------------------------------------------------

CHECKS = {
    "test_a_tone_comes_out_at_its_offset_from_the_tuned_centre": check_tone,
    "test_a_stream_cut_into_calls_is_the_uncut_stream": check_cuts,
    "test_restatement_against_the_definition": check_against_the_definition,
    "test_every_sample_is_rotated_at_its_own_stream_index": check_every_sample_is_rotated_at_its_own_stream_index,
    "test_a_null_history_is_a_history_of_zeros": check_null_history,
}
NAMED = {
    "conjugate": "test_a_tone_comes_out_at_its_offset_from_the_tuned_centre",
    "call_index": "test_a_stream_cut_into_calls_is_the_uncut_stream",
    "no_phase0": "test_restatement_against_the_definition",
    "rotate_output": "test_every_sample_is_rotated_at_its_own_stream_index",
    "raw_zeros": "test_a_null_history_is_a_history_of_zeros",
}


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
    for mu in tr.MUTANTS:
        marks = ["x" if _fails(CHECKS[n], mu) else "." for n in names]
        caught[mu] = marks[names.index(NAMED[mu])] == "x"
        rows.append("%-13s " % mu + "  ".join(marks) + "    T%d" % (names.index(NAMED[mu]) + 1))
    legend = ["  T%d = %s" % (i + 1, n) for i, n in enumerate(names)]
    return "\n".join(legend + [""] + rows), caught


def test_every_mutant_is_caught_by_its_named_test():
    assert set(NAMED) == set(tr.MUTANTS)
    table, caught = mutation_table()
    print(table)
    assert all(caught.values()), caught
    txt = open(os.path.join(ROOT, "profiles", "tune_mutations.txt")).read()
    for mu in tr.MUTANTS:
        assert mu in txt and NAMED[mu] in txt


# ---- through the oracle: channels 1 / 6 / 11 out of one capture ----------------------------------------------------------

def decoded(x, n_sym, plen):
    """the PSDUs of the FCS-good frames of a stream, in order, through the oracle's receiver"""
    prm = orc.make_params(max_sym=n_sym)
    o = orc.demod_stream(np.asarray(x, dtype=np.complex64), prm, cap=256)
    psdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
    ok = (o["frames"]["flags"] & capi.F_CRC_OK) != 0
    return psdu[ok][:, :plen]


def lost_per_channel(enc, plen, snr_db, db_up):
    wide, psdus, n_sym = tr.three_channel_scene(enc, plen, snr_db, db_up=db_up)
    y = tr.stream(wide, 4, 1, tr.scene_incs(), n_out=len(wide) // 4)
    got = [decoded(y[k], n_sym, plen) for k in range(3)]
    lost = [len(p) - sum(any(np.array_equal(g, q) for g in got[k]) for q in p) for k, p in enumerate(psdus)]
    return got, psdus, lost


@pytest.mark.parametrize("enc,plen,snr_db", [(7, 300, 28.0), (2, 100, 15.0)], ids=["qam64_34", "qpsk12"])
def test_three_channels_out_of_one_capture(enc, plen, snr_db):
    """every PSDU of every channel, in order, with the three at equal power; the outer two 20 dB up is printed only"""
    got, psdus, lost = lost_per_channel(enc, plen, snr_db, 0.0)
    print("encoding %d at %.0f dB: lost per channel %s of %d" % (enc, snr_db, lost, len(psdus[0])))
    for k in range(3):
        assert got[k].shape == psdus[k].shape and np.array_equal(got[k], psdus[k]), k
    _, _, lost20 = lost_per_channel(enc, plen, snr_db, 20.0)
    print("encoding %d at %.0f dB, outer channels +20 dB: lost per channel %s of %d" % (enc, snr_db, lost20, len(psdus[0])))
