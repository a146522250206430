"""NUMERICS.md rule 20 (tests/convert_ref.py) on the CPU: exactness, rounding, saturation, the special values and the error
bound -- and, through the oracle, the condition the device's stream test rests on."""
import numpy as np
import pytest

import convert_ref as cr

ALL = {cr.SC16: np.arange(-32768, 32768, dtype=np.int32).astype(np.int16), cr.SC8: np.arange(-128, 128, dtype=np.int32).astype(np.int8)}


@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8])
@pytest.mark.parametrize("log2_scale", [-15, -7, 0, 3])
def test_widening_is_exact_for_powers_of_two_and_round_trips(fmt, log2_scale):
    q = ALL[fmt]
    scale = np.float32(2.0 ** log2_scale)
    v = cr.widen(q, scale)
    assert v.dtype == np.float32
    assert np.array_equal(v.astype(np.float64), q.astype(np.float64) * 2.0 ** log2_scale)      # exact
    back, clipped = cr.quantise(v, np.float32(2.0 ** -log2_scale), fmt)
    assert back.dtype == q.dtype and np.array_equal(back, q) and clipped == 0


@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8])
def test_ties_go_to_even(fmt):
    x = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5], np.float32)
    q, clipped = cr.quantise(x, 1.0, fmt)
    assert q.tolist() == [0, 0, 2, -2, 2, -2] and clipped == 0
    q, _ = cr.quantise(x * np.float32(4), 0.25, fmt)      # the tie arises in the product
    assert q.tolist() == [0, 0, 2, -2, 2, -2]


@pytest.mark.parametrize("fmt,bits", [(cr.SC16, 2), (cr.SC16, 8), (cr.SC16, 12), (cr.SC16, 16), (cr.SC8, 2), (cr.SC8, 8)])
def test_saturation_at_both_ends(fmt, bits):
    lo, hi = -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
    x = np.array([hi - 1, hi, hi + 0.49, hi + 0.5, hi + 1, 1e9, lo + 1, lo, lo - 0.5, lo - 0.51, lo - 1, -1e9], np.float32)
    q, clipped = cr.quantise(x, 1.0, fmt, bits)
    # hi + 0.5 rounds to the even hi + 1 and clips; lo - 0.5 rounds to the even lo and does not.  (At 16 bits float32 still
    # holds the halves: 32767.5 and -32768.5 are exact.)
    assert q.tolist() == [hi - 1, hi, hi, hi, hi, hi, lo + 1, lo, lo, lo, lo, lo]
    assert clipped == 3 + 3


def test_special_values_and_the_clip_count():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([[nan, 1.0], [inf, -inf], [0.0, -0.0], [127.0, 128.0], [-128.0, -129.0], [3e38, nan]], np.float32)
    q, clipped = cr.quantise(x, 1.0, cr.SC8)
    assert q.tolist() == [[0, 1], [127, -128], [0, 0], [127, 127], [-128, -128], [127, 0]]
    assert clipped == 1 + 2 + 0 + 1 + 1 + 2             # I and Q each count on their own
    q, clipped = cr.quantise(x, 4.0, cr.SC16)           # 3e38 * 4 overflows to +inf in the float32 product: saturates
    assert q.tolist() == [[0, 4], [32767, -32768], [0, 0], [508, 512], [-512, -516], [32767, 0]]
    assert clipped == 1 + 2 + 0 + 0 + 0 + 2


@pytest.mark.parametrize("fmt,bits", [(cr.SC16, 16), (cr.SC16, 12), (cr.SC8, 8), (cr.SC8, 4)])
def test_round_trip_error_is_half_a_step_where_nothing_clipped(fmt, bits):
    rng = np.random.default_rng(20)
    x = rng.standard_normal(1 << 16).astype(np.float32)
    scale = np.float32(2.0 ** (bits - 1) / 3.0)          # full scale at 3 sigma: 0.3 % of the samples clip
    q, clipped = cr.quantise(x, scale, fmt, bits)
    t = x.astype(np.float64) * float(scale)
    inside = (np.rint(t) >= -(2 ** (bits - 1))) & (np.rint(t) <= 2 ** (bits - 1) - 1)
    assert clipped == np.count_nonzero(~inside) and 0 < clipped < x.size // 100
    back = cr.widen(q, 1.0).astype(np.float64) / float(scale)
    # |widen(quantise(x)) * 1 - x * scale| <= 0.5, i.e. 0.5 / scale in x's unit; the float32 product adds 2^-24 relative
    assert np.all(np.abs(back - x.astype(np.float64))[inside] <= (0.5 + 2.0 ** -24 * np.abs(t[inside])) / float(scale))


@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8])
def test_stream_condition(orc, fmt):
    """What tests/test_gpu_stream_formats.py rests on: the test stream, quantised on the host at 12 dB back-off and widened
    again, still carries every transmitted frame with a good FCS -- sc8 at 64-QAM 3/4 included, so neither arm needs the
    16-QAM fall-back."""
    import stream_formats_case as case
    x, psdus, q, scale_q, w, scale_w = case.stream(fmt)
    assert 10000 < x.size < 13000 and q.shape == (x.size, 2) and q.dtype == cr.DTYPE[fmt]
    assert np.abs(q.astype(np.int32)).max() >= 2 ** (cr.MAX_BITS[fmt] - 1) // 2      # the back-off is what it says: the peaks come near full scale
    o, psdu = case.oracle_result(fmt)
    fr = o["frames"]
    ok = (fr["flags"] & orc.F_CRC_OK) != 0
    assert len(fr) == len(psdus) and ok.all()
    assert fr["encoding"].tolist() == list(case.RATES[fmt])
    for k, p in enumerate(psdus):
        assert np.array_equal(psdu[k, :len(p)], p)
