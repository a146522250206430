"""wifirx_arb_resample (wr_arb.hip) against tests/arb_ref.py, bit for bit: every ratio of the rule's list, every size around the
history and the kernel's tile, every sample format, both input offsets, the output between canaries, hist and hist_out, the
start of a stream and a place 2^50 samples into it, a stream cut into calls, two calls queued back to back, one large call,
non-finite samples, and the refused arguments."""
import ctypes as C

import numpy as np
import pytest

import arb_ref as ar
import convert_ref as cr
from bank_helpers import CANARY, alloc_bufs, bits_of, download_fenced, fill, open_rx, same_bits, tile
from wifirx import capi

pytestmark = pytest.mark.gpu

T = tile("wr_arb.h", "WR_ARB_TILE")
BPS = {cr.FC32: 8, cr.SC16: 4, cr.SC8: 2}
FORMATS = [cr.FC32, cr.SC16, cr.SC8]
FMT_ID = {cr.FC32: "fc32", cr.SC16: "sc16", cr.SC8: "sc8"}
CASES = [pytest.param(num, den, fmt, id="%d_%d-%s" % (num, den, FMT_ID[fmt])) for num, den in ar.RATIOS for fmt in FORMATS]
FAR = (1 << 50) + 12345


def inputs_for(num, den, n_out):
    """the fewest inputs of a stream from 0 that make n_out outputs"""
    return ar.flush_inputs(num, den, 0, n_out)


def sizes(num, den):
    HL = ar.hist_len(num, den)
    return (0, 1, 2, HL - 1, HL, HL + 1, inputs_for(num, den, T - 1), inputs_for(num, den, T), inputs_for(num, den, T + 1),
            inputs_for(num, den, 2 * T + 3), 1031)


N_IN_MAX = max(max(sizes(n, d)) for n, d in ar.RATIOS)
N_OUT_MAX = max(ar.count(n, d, 0, N_IN_MAX + ar.HIST_MAX, 0) for n, d in ar.RATIOS) + 8
# (input offset in samples, hist given, j0, scale of the integer formats): both offsets, hist NULL and given, the start of a
# stream (where hist lies in front of the stream and reads as zeros) and a place far into one
COMBOS = ((0, False, 0, None), (1, True, FAR, 1.0 / 3.0), (0, False, FAR, 2.0 ** -3), (1, True, 0, None))


@pytest.fixture(scope="module")
def rx():
    yield from open_rx()


@pytest.fixture(scope="module")
def bufs(rx):
    yield from alloc_bufs(rx, inp=(N_IN_MAX + 1) * 8 + 16, hist=ar.HIST_MAX * 8, hout=ar.HIST_MAX * 8 + 32, hout2=ar.HIST_MAX * 8,
                          out=24 + N_OUT_MAX * 8 + 64)


def samples(rng, n, fmt):
    """n samples of a format, [n, 2]"""
    if fmt == cr.FC32:
        return rng.standard_normal((n, 2)).astype(np.float32)
    info = np.iinfo(cr.DTYPE[fmt])
    return rng.integers(info.min, info.max + 1, (n, 2)).astype(cr.DTYPE[fmt])


def scale_of(fmt, scale):
    if fmt == cr.FC32:
        return float("nan")                                   # not looked at
    return float(cr.SCALE[fmt] if scale is None else np.float32(scale))


def m0_of(num, den, j0):
    """the output index of a stream whose calls so far took the inputs [0, j0)"""
    return ar.m_end(num, den, j0)


def run_dev(rx, bufs, x, fmt, num, den, hist, j0, m0, scale, in_off=0, want_hist_out=True):
    """one call at the test's offsets: the outputs as float32 pairs [n_out, 2] and hist_out (the format's dtype, [HL, 2]);
    checks n_out, every byte of the output allocation outside the outputs, and the bytes behind hist_out"""
    bps, n_in, HL = BPS[fmt], len(x), ar.hist_len(num, den)
    want_n = ar.count(num, den, j0, n_in, m0)
    bufs["inp"].upload(np.concatenate([np.full(in_off * bps, 0x5A, np.uint8), bits_of(x), np.full(16, 0x5A, np.uint8)]))
    if hist is not None:
        bufs["hist"].upload(bits_of(hist))
    fill(bufs["out"])
    fill(bufs["hout"])
    assert bufs["out"].ptr % 16 == 0
    n_out = rx.arb_resample_dev(bufs["inp"].ptr + in_off * bps, fmt, n_in, num, den, bufs["out"].ptr + 24, want_n,
                                hist_ptr=None if hist is None else bufs["hist"].ptr,
                                hist_out_ptr=bufs["hout"].ptr if want_hist_out else None, j0=j0, m0=m0, scale=scale_of(fmt, scale))
    assert n_out == want_n
    raw = download_fenced(bufs["out"], [(24, n_out * 8)], "its outputs")
    y = raw[24:24 + n_out * 8].view(np.float32).reshape(-1, 2)
    nh = HL * bps if want_hist_out else 0
    hraw = download_fenced(bufs["hout"], [(0, nh)], "hist_out")
    dt = np.float32 if fmt == cr.FC32 else cr.DTYPE[fmt]
    return y, hraw[:nh].view(dt).reshape(-1, 2)


@pytest.mark.parametrize("num,den,fmt", CASES)
def test_sizes_offsets_hist_and_place(rx, bufs, num, den, fmt):
    rng = np.random.default_rng(1000 * num + 10 * den + fmt)
    HL = ar.hist_len(num, den)
    for n_in in sizes(num, den):
        x = samples(rng, n_in, fmt)
        h = samples(rng, HL, fmt)
        for in_off, with_hist, j0, scale in COMBOS:
            hist, m0 = (h if with_hist else None), m0_of(num, den, j0)
            got, hout = run_dev(rx, bufs, x, fmt, num, den, hist, j0, m0, scale, in_off)
            want = ar.resample_format(x, fmt, scale_of(fmt, scale), num, den, hist, j0, m0)
            assert same_bits(got, want), (n_in, in_off, with_hist, j0)
            assert same_bits(hout, ar.next_history(x, hist, num, den)), (n_in, in_off, with_hist)


@pytest.mark.parametrize("num,den,fmt", CASES)
def test_a_stream_cut_into_calls_is_the_uncut_stream(rx, bufs, num, den, fmt):
    """hist_out of a call as the next call's hist, j0 and m0 advanced by its inputs and outputs: byte-identical -- one stream
    in three calls cut at 1 and HL inputs, and in two cut at the inputs of a tile plus one output"""
    rng = np.random.default_rng(77 * num + den + 3 * fmt)
    HL = ar.hist_len(num, den)
    n_in = inputs_for(num, den, 2 * T + 3)
    x = samples(rng, n_in, fmt)
    whole, hist_end = run_dev(rx, bufs, x, fmt, num, den, None, 0, 0, None)
    assert same_bits(whole, ar.resample_format(x, fmt, scale_of(fmt, None), num, den))
    for cuts in ((1, HL), (inputs_for(num, den, T + 1),)):
        hist, parts, pos, m0 = None, [], 0, 0
        for end in cuts + (n_in,):
            y, hist = run_dev(rx, bufs, x[pos:end], fmt, num, den, hist, pos, m0, None)
            parts.append(y)
            pos, m0 = end, m0 + len(y)
        assert same_bits(np.concatenate(parts), whole), cuts
        assert same_bits(hist, hist_end), cuts


def test_two_calls_queued_without_a_sync(rx, bufs):
    """the same through device pointers alone: hist_out of call one is hist of call two, in the second of two buffers, and
    nothing waits between the calls"""
    num, den, fmt, n1, n2 = 192, 125, cr.SC16, 300, 500
    x = samples(np.random.default_rng(5), n1 + n2, fmt)
    HL = ar.hist_len(num, den)
    d_in, d_out = bufs["inp"], bufs["out"]
    d_in.upload(bits_of(x))
    total = ar.count(num, den, 0, n1 + n2, 0)
    m1 = rx.arb_resample_dev(d_in.ptr, fmt, n1, num, den, d_out.ptr, total, hist_out_ptr=bufs["hout"].ptr)
    m2 = rx.arb_resample_dev(d_in.ptr + n1 * 4, fmt, n2, num, den, d_out.ptr + m1 * 8, total - m1, hist_ptr=bufs["hout"].ptr,
                             hist_out_ptr=bufs["hout2"].ptr, j0=n1, m0=m1)
    assert m1 + m2 == total
    got = d_out.download(np.float32, 2 * total).reshape(-1, 2)
    assert same_bits(got, ar.resample_format(x, fmt, cr.SCALE[fmt], num, den))
    assert same_bits(bufs["hout2"].download(np.int16, HL * 2).reshape(-1, 2), x[-HL:])


def test_no_input_still_hands_on_the_history(rx, bufs):
    num, den, fmt = 4, 1, cr.SC8
    h = samples(np.random.default_rng(6), ar.hist_len(num, den), fmt)
    got, hout = run_dev(rx, bufs, h[:0], fmt, num, den, h, FAR, m0_of(num, den, FAR), None)
    assert got.shape == (0, 2) and same_bits(hout, h)
    got, hout = run_dev(rx, bufs, h[:0], fmt, num, den, None, FAR, m0_of(num, den, FAR), None)
    assert same_bits(hout, np.zeros_like(h))
    # fewer inputs than the history holds: the tail of hist, then the inputs
    x = samples(np.random.default_rng(7), 5, fmt)
    got, hout = run_dev(rx, bufs, x, fmt, num, den, h, FAR, m0_of(num, den, FAR), None)
    assert same_bits(hout, np.concatenate([h[5:], x]))
    # and with neither input nor hist_out, NULL in and out are taken
    n = C.c_uint64(99)
    assert capi.lib().wifirx_arb_resample(rx._h, None, fmt, 1.0, 0, None, None, num, den, 0, 0, None, 0, C.byref(n)) == capi.OK
    assert n.value == 0


def test_an_unreduced_ratio_gives_the_reduced_ones_bytes(rx, bufs):
    x = samples(np.random.default_rng(8), 700, cr.FC32)
    a, ha = run_dev(rx, bufs, x, cr.FC32, 10, 8, None, 0, 0, None)
    b, hb = run_dev(rx, bufs, x, cr.FC32, 5, 4, None, 0, 0, None)
    assert len(a) and same_bits(a, b) and same_bits(ha, hb)
    one, _ = run_dev(rx, bufs, x, cr.FC32, 7, 7, None, 0, 0, None)
    assert same_bits(one, x[:len(one)]) and len(one) == 700 - 16


def test_one_large_call(rx):
    """2^20 inputs at 5/4: 4096 sampled outputs, the first and last ones included"""
    num, den, fmt, n_in = 5, 4, cr.FC32, 1 << 20
    rng = np.random.default_rng(9)
    x = rng.standard_normal((n_in, 2)).astype(np.float32)
    n_out = ar.count(num, den, 0, n_in, 0)
    pick = np.unique(np.concatenate([rng.integers(0, n_out, 4096 - 64), np.arange(32), np.arange(n_out - 32, n_out)]))
    d_in, d_out = rx.alloc(x.nbytes), rx.alloc(n_out * 8)
    try:
        d_in.upload(x)
        assert rx.arb_resample_dev(d_in.ptr, fmt, n_in, num, den, d_out.ptr, n_out) == n_out
        got = d_out.download(np.float32, 2 * n_out).reshape(-1, 2)[pick]
    finally:
        d_in.free()
        d_out.free()
    assert same_bits(got, ar.resample(x, num, den, outputs=pick))


@pytest.mark.parametrize("num,den", [(1, 1), (5, 4), (4, 5), (4, 1)])
def test_non_finite_samples(rx, bufs, num, den):
    """NaN and infinities among the samples: the same outputs are non-finite as in the restatement, every other output is
    bit-equal"""
    rng = np.random.default_rng(10 + num)
    x = samples(rng, 900, cr.FC32)
    x[100, 0], x[300, 1], x[301, 0], x[650, 1] = np.nan, np.inf, -np.inf, np.nan
    got, _ = run_dev(rx, bufs, x, cr.FC32, num, den, None, 0, 0, None)
    want = ar.resample(x, num, den)
    assert got.shape == want.shape
    bad = ~np.isfinite(want)
    assert bad.any() and not bad.all()
    assert np.array_equal(~np.isfinite(got), bad)
    assert np.array_equal(bits_of(got[~bad]), bits_of(want[~bad]))


def test_refused_arguments_leave_every_buffer_alone(rx, bufs):
    lib, h = capi.lib(), rx._h
    nan, inf = float("nan"), float("inf")
    i, hi, ho, o = bufs["inp"].ptr, bufs["hist"].ptr, bufs["hout"].ptr, bufs["out"].ptr
    big = rx.alloc(1 << 16)
    b = big.ptr
    n = 400                                                   # 5/4: 304 outputs, HL = 40
    n_out = ar.count(5, 4, 0, n, 0)
    far_m = m0_of(5, 4, FAR)
    # (in, fmt, scale, n_in, hist, hist_out, num, den, j0, m0, out, out_cap)
    einval = [
        (None, 0, 1.0, n, hi, ho, 5, 4, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 0, 0, None, n),
        (i, 3, 1.0, n, hi, ho, 5, 4, 0, 0, o, n), (i, -1, 1.0, n, hi, ho, 5, 4, 0, 0, o, n),
        (i, 1, 0.0, n, hi, ho, 5, 4, 0, 0, o, n), (i, 2, -1.0, n, hi, ho, 5, 4, 0, 0, o, n), (i, 1, nan, n, hi, ho, 5, 4, 0, 0, o, n),
        (i, 2, inf, n, hi, ho, 5, 4, 0, 0, o, n),
        (i, 0, 1.0, n, hi, ho, 0, 4, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 0, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 1, 0, 0, o, n),
        (i, 0, 1.0, n, hi, ho, 1, 5, 0, 0, o, 8 * n), (i, 0, 1.0, n, hi, ho, 1027, 513, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 2049, 1024, 0, 0, o, n),
        (i + 4, 0, 1.0, n, hi, ho, 5, 4, 0, 0, o, n), (i + 2, 1, 1.0, n, hi, ho, 5, 4, 0, 0, o, n), (i + 1, 2, 1.0, n, hi, ho, 5, 4, 0, 0, o, n),
        (i, 0, 1.0, n, hi + 4, ho, 5, 4, 0, 0, o, n), (i, 1, 1.0, n, hi, ho + 2, 5, 4, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 0, 0, o + 4, n),
        # overlaps: in / out, out's last byte / in, hist / out, hist_out / out, hist_out / in, hist_out / hist, hist / in
        (b, 0, 1.0, n, None, None, 5, 4, 0, 0, b, n), (b + n_out * 8 - 8, 0, 1.0, n, None, None, 5, 4, 0, 0, b, n),
        (i, 0, 1.0, n, b, None, 5, 4, FAR, far_m, b + 8, n), (i, 0, 1.0, n, None, b + n_out * 8 - 8, 5, 4, 0, 0, b, n),
        (b, 0, 1.0, n, None, b + n * 8 - 8, 5, 4, 0, 0, o, n), (i, 0, 1.0, n, b, b + 40 * 8 - 8, 5, 4, FAR, far_m, o, n),
        (b + 40 * 2 - 2, 2, 1.0, n, b, None, 5, 4, FAR, far_m, o, n), (i, 0, 1.0, n, hi, hi, 5, 4, 0, 0, o, n),
        # a history that does not reach: the call's first output starts more than HL samples in front of in[0]
        (i, 0, 1.0, n, hi, ho, 5, 4, 1000, 0, o, 8 * n), (i, 0, 1.0, n, hi, ho, 5, 4, FAR, far_m - 2, o, n),
        (i, 0, 1.0, n, None, ho, 4, 1, FAR, m0_of(4, 1, FAR) - 2, o, n),
    ]
    erange = [
        (i, 0, 1.0, n, hi, ho, 5, 4, 0, 0, o, n_out - 1), (i, 0, 1.0, n, hi, ho, 5, 4, 0, 0, o, 0),
        (i, 0, 1.0, n, hi, ho, 5, 4, (1 << 60) - n, 0, o, n), (i, 0, 1.0, n, hi, ho, 1, 1, (1 << 62) - n, 0, o, n),
        (i, 0, 1.0, (1 << 64) - 1, hi, ho, 1, 1, 1 << 63, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 0, 1 << 60, o, n),
        (i, 0, 1.0, n, hi, ho, 1, 4, (1 << 59) - n, 0, o, 8 * n),
    ]
    try:
        fills = {k: fill(d) for k, d in bufs.items()}
        fill(big)
        made = C.c_uint64(77)
        for a in einval:
            assert lib.wifirx_arb_resample(h, *a, C.byref(made)) == capi.EINVAL, a
        for a in erange:
            assert lib.wifirx_arb_resample(h, *a, C.byref(made)) == capi.ERANGE, a
        assert lib.wifirx_arb_resample(h, i, 0, 1.0, n, hi, ho, 5, 4, 0, 0, o, n, None) == capi.EINVAL
        assert made.value == 77
        rx.sync()
        for k, d in bufs.items():
            assert np.array_equal(d.download(np.uint8, d.nbytes), fills[k]), k
        assert (big.download(np.uint8, 1 << 16) == CANARY).all()
        # buffers that only touch are taken: hist, in, hist_out and out one behind the other
        n_h = 40 * 8
        assert lib.wifirx_arb_resample(h, b + n_h, 0, 1.0, n, b, b + n_h + n * 8, 5, 4, 0, 0, b + 2 * n_h + n * 8, n_out,
                                       C.byref(made)) == capi.OK
        assert made.value == n_out
        rx.sync()
    finally:
        big.free()
