"""wifirx_tune (wr_arb.hip, tune_kernel) against tests/tune_ref.py, bit for bit: five ratios, every sample format, 1, 3 and 8
channels, output counts around the kernel's tile, both input offsets, hist NULL and given, the start of a stream and a place
2^50 samples into it, rows further apart than their outputs with canaries between them, a channel at the capture's centre
against wifirx_arb_resample itself, a stream cut into calls, two calls queued back to back, rotated zeros, non-finite
samples, and the refused arguments."""
import ctypes as C

import numpy as np
import pytest

import arb_ref as ar
import convert_ref as cr
import tune_ref as tr
from bank_helpers import CANARY, alloc_bufs, bits_of, download_fenced, fill, open_rx, same_bits, tile
from wifirx import capi

pytestmark = pytest.mark.gpu

T = tile("wr_arb.h", "WR_ARB_TILE")
BPS = {cr.FC32: 8, cr.SC16: 4, cr.SC8: 2}
FORMATS = [cr.FC32, cr.SC16, cr.SC8]
FMT_ID = {cr.FC32: "fc32", cr.SC16: "sc16", cr.SC8: "sc8"}
RATIOS = ((1, 1), (5, 4), (4, 5), (4, 1), (384, 125))
CASES = [pytest.param(num, den, fmt, id="%d_%d-%s" % (num, den, FMT_ID[fmt])) for num, den in RATIOS for fmt in FORMATS]
COUNTS = (1, T - 1, T, T + 1, 1000)
FAR = (1 << 50) + 12345
INC_UP, INC_DOWN = 0x5000000000000000, 0xB000000000000000    # channels at -25 and +25 MHz of an 80 MS/s capture
PH = 0x3243F6A8885A308D
# (input offset in samples, hist given, j0, scale of the integer formats, float pairs between a row's end and the next row)
COMBOS = ((0, False, 0, None, 0), (1, True, FAR, 1.0 / 3.0, 3), (0, False, FAR, 2.0 ** -3, 1), (1, True, 0, None, 0))
N_IN_MAX, ROW_MAX = 8192, 6000


def channels(K, seed):
    """(incs, phase0s) of a call: the outer channels of the band, the centre among them from K = 3, random ones beyond"""
    rng = np.random.default_rng(seed)
    if K == 1:
        return [INC_DOWN + 12345], [PH]
    incs, phs = [INC_UP, 0, INC_DOWN], [0, 0, PH]
    while len(incs) < K:
        incs.append(int(rng.integers(0, 1 << 63)) * 2 + 1)
        phs.append(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)))
    return incs, phs


@pytest.fixture(scope="module")
def rx():
    yield from open_rx()


@pytest.fixture(scope="module")
def bufs(rx):
    yield from alloc_bufs(rx, inp=(N_IN_MAX + 1) * 8 + 16, hist=ar.HIST_MAX * 8, hout=ar.HIST_MAX * 8 + 32, hout2=ar.HIST_MAX * 8,
                          out=24 + tr.MAX_CHANNELS * ROW_MAX * 8 + 64)


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


def call_for(num, den, j0, n_out):
    """(n_in, m0): the fewest inputs behind j0 that complete n_out outputs beyond m_end(j0), and the first of the last n_out"""
    base = ar.m_end(num, den, j0)
    n_in = max(0, (n_out * num) // den - 2)
    while ar.m_end(num, den, j0 + n_in) - base < n_out:
        n_in += 1
    return n_in, ar.m_end(num, den, j0 + n_in) - n_out


def run_dev(rx, bufs, x, fmt, num, den, incs, phs, hist, j0, m0, scale, in_off=0, gap=0, want_hist_out=True):
    """one call at the test's offsets: the outputs as float32 pairs [K, n_out, 2] and hist_out (the format's dtype, [HL, 2]);
    checks n_out, every byte of the output allocation outside the rows' outputs, and the bytes behind hist_out"""
    bps, n_in, HL, K = BPS[fmt], len(x), ar.hist_len(num, den), len(incs)
    want_n = ar.count(num, den, j0, n_in, m0)
    stride = want_n + gap
    assert K * stride <= tr.MAX_CHANNELS * ROW_MAX and n_in <= N_IN_MAX
    bufs["inp"].upload(np.concatenate([np.full(in_off * bps, 0x5A, np.uint8), bits_of(x), np.full(16, 0x5A, np.uint8)]))
    if hist is not None:
        bufs["hist"].upload(bits_of(hist))
    fill(bufs["out"])
    fill(bufs["hout"])
    n_out = rx.tune_dev(bufs["inp"].ptr + in_off * bps, fmt, n_in, num, den, incs, bufs["out"].ptr + 24, stride, phase0s=phs,
                        hist_ptr=None if hist is None else bufs["hist"].ptr,
                        hist_out_ptr=bufs["hout"].ptr if want_hist_out else None, j0=j0, m0=m0, scale=scale_of(fmt, scale))
    assert n_out == want_n
    raw = download_fenced(bufs["out"], [(24 + k * stride * 8, n_out * 8) for k in range(K)], "its rows' outputs")
    y = np.stack([raw[24 + k * stride * 8:24 + k * stride * 8 + n_out * 8].view(np.float32).reshape(-1, 2) for k in range(K)])
    nh = HL * bps if want_hist_out else 0
    hraw = download_fenced(bufs["hout"], [(0, nh)], "hist_out")
    dt = np.float32 if fmt == cr.FC32 else cr.DTYPE[fmt]
    return y, hraw[:nh].view(dt).reshape(-1, 2)


@pytest.mark.parametrize("num,den,fmt", CASES)
def test_channels_counts_offsets_hist_and_place(rx, bufs, num, den, fmt):
    rng = np.random.default_rng(1000 * num + 10 * den + fmt)
    HL = ar.hist_len(num, den)
    h = samples(rng, HL, fmt)
    step, seen_short = 0, False
    for K in (1, 3, 8):
        incs, phs = channels(K, 7 * K + num)
        for n_out in COUNTS:
            in_off, with_hist, j0, scale, gap = COMBOS[step % len(COMBOS)]
            step += 1
            n_in, m0 = call_for(num, den, j0, n_out)
            seen_short |= n_in < HL
            x = samples(rng, n_in, fmt)
            hist = h if with_hist else None
            got, hout = run_dev(rx, bufs, x, fmt, num, den, incs, phs, hist, j0, m0, scale, in_off, gap)
            want = tr.tune_format(x, fmt, scale_of(fmt, scale), num, den, incs, phs, hist, j0, m0)
            assert got.shape[1] == n_out and same_bits(got, want), (K, n_out, in_off, with_hist, j0, gap)
            assert same_bits(hout, ar.next_history(x, hist, num, den)), (K, n_out)
    if (num, den) == (4, 1):
        assert seen_short                                     # one output of 4/1 needs 65 inputs, fewer than the history holds


@pytest.mark.parametrize("num,den,fmt", [(4, 1, cr.SC16), (384, 125, cr.FC32), (1, 1, cr.SC8)], ids=["4_1-sc16", "384_125-fc32", "1_1-sc8"])
def test_a_centre_channel_is_wifirx_arb_resample(rx, bufs, num, den, fmt):
    """the middle row of a three-channel call and a wifirx_arb_resample call on the same buffers: the same bytes"""
    rng = np.random.default_rng(11 * num + fmt)
    HL = ar.hist_len(num, den)
    n_in, m0 = call_for(num, den, FAR, 700)
    x, h = samples(rng, n_in, fmt), samples(rng, HL, fmt)
    got, _ = run_dev(rx, bufs, x, fmt, num, den, [INC_UP, 0, INC_DOWN], [PH, 0, 0], h, FAR, m0, None)
    n = got.shape[1]
    fill(bufs["out"])
    assert rx.arb_resample_dev(bufs["inp"].ptr, fmt, n_in, num, den, bufs["out"].ptr + 24, n, hist_ptr=bufs["hist"].ptr, j0=FAR,
                               m0=m0, scale=scale_of(fmt, None)) == n
    raw = download_fenced(bufs["out"], [(24, n * 8)], "its outputs")
    plain = raw[24:24 + n * 8].view(np.float32).reshape(-1, 2)
    assert same_bits(got[1], plain)
    assert not same_bits(got[0], plain) and not same_bits(got[2], plain)


@pytest.mark.parametrize("num,den,fmt", [(4, 1, cr.FC32), (5, 4, cr.SC16), (4, 5, cr.SC8)], ids=["4_1-fc32", "5_4-sc16", "4_5-sc8"])
def test_a_stream_cut_into_calls_is_the_uncut_stream(rx, bufs, num, den, fmt):
    """hist_out of a call as the next call's hist, j0 and m0 advanced by its inputs and outputs, the increments and phases
    left alone: byte-identical -- one stream in calls of 1, 257 and 4096 inputs and the rest"""
    rng = np.random.default_rng(77 * num + den + 3 * fmt)
    n_in = 1 + 257 + 4096 + 300
    x = samples(rng, n_in, fmt)
    incs, phs = [INC_UP, 0, INC_DOWN + 999], [PH, 0, 1]
    whole, hist_end = run_dev(rx, bufs, x, fmt, num, den, incs, phs, None, 0, 0, None)
    assert same_bits(whole, tr.tune_format(x, fmt, scale_of(fmt, None), num, den, incs, phs))
    hist, parts, pos, m0 = None, [], 0, 0
    for end in (1, 1 + 257, 1 + 257 + 4096, n_in):
        y, hist = run_dev(rx, bufs, x[pos:end], fmt, num, den, incs, phs, hist, pos, m0, None, gap=end % 3)
        parts.append(y)
        pos, m0 = end, m0 + y.shape[1]
    assert same_bits(np.concatenate(parts, axis=1), whole)
    assert same_bits(hist, hist_end)


def test_two_calls_queued_without_a_sync(rx, bufs):
    """the same through device pointers alone: hist_out of call one is hist of call two, in the second of two buffers, and
    nothing waits between the calls"""
    num, den, fmt, n1, n2 = 4, 1, cr.SC16, 700, 1100
    x = samples(np.random.default_rng(5), n1 + n2, fmt)
    HL = ar.hist_len(num, den)
    incs, phs = [INC_UP, 0, INC_DOWN], [1 << 62, 0, PH]
    d_in, d_out = bufs["inp"], bufs["out"]
    d_in.upload(bits_of(x))
    total = ar.count(num, den, 0, n1 + n2, 0)
    m1 = rx.tune_dev(d_in.ptr, fmt, n1, num, den, incs, d_out.ptr, total, phase0s=phs, hist_out_ptr=bufs["hout"].ptr)
    m2 = rx.tune_dev(d_in.ptr + n1 * 4, fmt, n2, num, den, incs, d_out.ptr + m1 * 8, total, phase0s=phs, hist_ptr=bufs["hout"].ptr,
                     hist_out_ptr=bufs["hout2"].ptr, j0=n1, m0=m1)
    assert m1 + m2 == total
    got = d_out.download(np.float32, 2 * total * 3).reshape(3, -1, 2)
    assert same_bits(got, tr.tune_format(x, fmt, cr.SCALE[fmt], num, den, incs, phs))
    assert same_bits(bufs["hout2"].download(np.int16, HL * 2).reshape(-1, 2), x[-HL:])


def test_zeros_are_rotated_like_any_sample(rx, bufs):
    """1/1 on a stretch of zero samples with the phase in the second quadrant: the outputs are (-0, +0), from a NULL history,
    from a history of zeros and in front of the stream alike, as in the restatement"""
    x = samples(np.random.default_rng(6), 100, cr.FC32)
    x[:40] = 0
    inc, ph = [1 << 40], [3 << 61]
    m0 = ar.m_end(1, 1, 1000)
    a, _ = run_dev(rx, bufs, x, cr.FC32, 1, 1, inc, ph, None, 1000, m0, None)
    b, _ = run_dev(rx, bufs, x, cr.FC32, 1, 1, inc, ph, np.zeros((32, 2), np.float32), 1000, m0, None)
    c, _ = run_dev(rx, bufs, x, cr.FC32, 1, 1, inc, ph, None, 0, 0, None)
    assert same_bits(a, b) and same_bits(a, tr.tune(x, 1, 1, inc, ph, None, 1000, m0))
    assert same_bits(c, tr.tune(x, 1, 1, inc, ph))
    for y in (a, c):
        assert np.signbit(y[0, :8, 0]).all() and not np.signbit(y[0, :8, 1]).any()


@pytest.mark.parametrize("num,den", [(1, 1), (5, 4), (4, 1)])
def test_non_finite_samples(rx, bufs, num, den):
    """NaN and infinities among the samples: the same outputs are non-finite as in the restatement, every other output is
    bit-equal; the centre channel's bytes are wifirx_arb_resample's on them too"""
    rng = np.random.default_rng(10 + num)
    x = samples(rng, 1300, cr.FC32)
    x[100, 0], x[300, 1], x[301, 0], x[650, 1] = np.nan, np.inf, -np.inf, np.nan
    incs, phs = [INC_UP, 0, INC_DOWN], [0, 0, PH]
    got, _ = run_dev(rx, bufs, x, cr.FC32, num, den, incs, phs, None, 0, 0, None)
    want = tr.tune(x, num, den, incs, phs)
    assert got.shape == want.shape
    bad = ~np.isfinite(want)
    assert bad.any() and not bad.all()
    assert np.array_equal(~np.isfinite(got), bad)
    assert np.array_equal(bits_of(got[~bad]), bits_of(want[~bad]))
    assert np.array_equal(np.isnan(got), np.isnan(want))


def test_refused_arguments_leave_every_buffer_alone(rx, bufs):
    lib, h = capi.lib(), rx._h
    nan, inf = float("nan"), float("inf")
    i, hi, ho, o = bufs["inp"].ptr, bufs["hist"].ptr, bufs["hout"].ptr, bufs["out"].ptr
    big = rx.alloc(1 << 16)
    b = big.ptr
    n = 400                                                   # 5/4: 304 outputs, HL = 40
    n_out = ar.count(5, 4, 0, n, 0)
    far_m = ar.m_end(5, 4, FAR)
    inc = (C.c_uint64 * 8)(INC_UP, 0, INC_DOWN, 1, 2, 3, 4, 5)
    ph = (C.c_uint64 * 8)()
    # (in, fmt, scale, n_in, hist, hist_out, num, den, n_channels, inc, phase0, j0, m0, out, out_stride)
    einval = [
        (None, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, None, n),
        (i, 3, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n), (i, -1, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n),
        (i, 1, 0.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n), (i, 2, -1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n),
        (i, 1, nan, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n), (i, 2, inf, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n),
        (i, 0, 1.0, n, hi, ho, 0, 4, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 0, 3, inc, ph, 0, 0, o, n),
        (i, 0, 1.0, n, hi, ho, 5, 1, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 1, 5, 3, inc, ph, 0, 0, o, 8 * n),
        (i, 0, 1.0, n, hi, ho, 1027, 513, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 2049, 1024, 3, inc, ph, 0, 0, o, n),
        (i + 4, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n), (i + 2, 1, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n),
        (i + 1, 2, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi + 4, ho, 5, 4, 3, inc, ph, 0, 0, o, n),
        (i, 1, 1.0, n, hi, ho + 2, 5, 4, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o + 4, n),
        # the channels
        (i, 0, 1.0, n, hi, ho, 5, 4, 0, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 9, inc, ph, 0, 0, o, n),
        (i, 0, 1.0, n, hi, ho, 5, 4, 3, None, ph, 0, 0, o, n),
        # overlaps: in / out, the last row's last byte / in, in / the room behind a row's outputs, hist / out, hist_out / out,
        # hist_out / in, hist_out / hist, hist / in
        (b, 0, 1.0, n, None, None, 5, 4, 3, inc, ph, 0, 0, b, n), (b + 3 * n * 8 - 8, 0, 1.0, n, None, None, 5, 4, 3, inc, ph, 0, 0, b, n),
        (b + n_out * 8, 0, 1.0, 10, None, None, 5, 4, 3, inc, ph, FAR, far_m, b, n),
        (i, 0, 1.0, n, b, None, 5, 4, 3, inc, ph, FAR, far_m, b + 8, n), (i, 0, 1.0, n, None, b + 3 * n * 8 - 8, 5, 4, 3, inc, ph, 0, 0, b, n),
        (b, 0, 1.0, n, None, b + n * 8 - 8, 5, 4, 3, inc, ph, 0, 0, o, n), (i, 0, 1.0, n, b, b + 40 * 8 - 8, 5, 4, 3, inc, ph, FAR, far_m, o, n),
        (b + 40 * 2 - 2, 2, 1.0, n, b, None, 5, 4, 3, inc, ph, FAR, far_m, o, n), (i, 0, 1.0, n, hi, hi, 5, 4, 3, inc, ph, 0, 0, o, n),
        # a history that does not reach
        (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 1000, 0, o, 8 * n), (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, FAR, far_m - 2, o, n),
    ]
    erange = [
        (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n_out - 1), (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, 0),
        (i, 0, 1.0, n, hi, ho, 5, 4, 1, inc, ph, 0, 0, o, n_out - 1), (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, 1 << 61),
        (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, (1 << 60) - n, 0, o, n), (i, 0, 1.0, n, hi, ho, 1, 1, 3, inc, ph, (1 << 62) - n, 0, o, n),
        (i, 0, 1.0, (1 << 64) - 1, hi, ho, 1, 1, 3, inc, ph, 1 << 63, 0, o, n), (i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 1 << 60, o, n),
        # more than 2^31 - 1 tiles (the count is taken before any buffer is looked at)
        (i, 0, 1.0, 1 << 40, hi, ho, 1, 1, 3, inc, ph, 0, 0, o, 1 << 41),
    ]
    try:
        fills = {k: fill(d) for k, d in bufs.items()}
        fill(big)
        made = C.c_uint64(77)
        for a in einval:
            assert lib.wifirx_tune(h, *a, C.byref(made)) == capi.EINVAL, a
        for a in erange:
            assert lib.wifirx_tune(h, *a, C.byref(made)) == capi.ERANGE, a
        assert lib.wifirx_tune(h, i, 0, 1.0, n, hi, ho, 5, 4, 3, inc, ph, 0, 0, o, n, None) == capi.EINVAL
        assert made.value == 77
        rx.sync()
        for k, d in bufs.items():
            assert np.array_equal(d.download(np.uint8, d.nbytes), fills[k]), k
        assert (big.download(np.uint8, 1 << 16) == CANARY).all()
        # buffers that only touch are taken: hist, in, hist_out and the three rows one behind the other; phase0 may be NULL
        n_h = 40 * 8
        assert lib.wifirx_tune(h, b + n_h, 0, 1.0, n, b, b + n_h + n * 8, 5, 4, 3, inc, None, 0, 0, b + 2 * n_h + n * 8, n_out,
                               C.byref(made)) == capi.OK
        assert made.value == n_out
        rx.sync()
    finally:
        big.free()
