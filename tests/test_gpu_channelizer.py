"""wifirx_channelize (wr_channelizer.hip) against tests/channelizer_ref.py, bit for bit: every size around the 24-tap window
and the kernel's tile, every channel count, stacking and sample format, both input offsets, rows between canaries, hist and
hist_out, a stream cut into calls, the parity of m0, one large call, and the refused arguments."""
import numpy as np
import pytest

import channelizer_ref as zr
import convert_ref as cr
from bank_helpers import CANARY, alloc_bufs, bits_of, download_fenced, fill, open_rx, same_bits, tile
from wifirx import capi

pytestmark = pytest.mark.gpu

T = tile("wr_channelizer.h", "WR_CZ_TILE")
SIZES = (0, 1, 2, 23, 24, 25, T - 1, T, T + 1, 2 * T + 3, 1031)
N_MAX = max(SIZES)
BPS = {cr.FC32: 8, cr.SC16: 4, cr.SC8: 2}
FORMATS = [cr.FC32, cr.SC16, cr.SC8]
FMT_ID = {cr.FC32: "fc32", cr.SC16: "sc16", cr.SC8: "sc8"}
CASES = [pytest.param(M, s, fmt, id="M%d-s%d-%s" % (M, s, FMT_ID[fmt])) for M in (2, 4, 8) for s in (0, 1) for fmt in FORMATS]
# (input offset in samples, hist given, m0, scale of the integer formats): both offsets, hist NULL and given, m0 even and odd
COMBOS = ((0, False, 0, None), (1, True, 7, 1.0 / 3.0), (0, True, (1 << 40) + 1, None), (1, False, 10, 2.0 ** -3))
OUT_ROOM = 16 + 8 + (8 * (N_MAX + 5)) * 8 + 64          # bytes: the lead, 8 rows of the largest stride, a margin


@pytest.fixture(scope="module")
def rx():
    yield from open_rx()


@pytest.fixture(scope="module")
def bufs(rx):
    yield from alloc_bufs(rx, inp=(N_MAX * 8 + 1) * 8 + 16, hist=23 * 8 * 8, hout=23 * 8 * 8 + 32, hout2=23 * 8 * 8, out=OUT_ROOM)


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


def run_dev(rx, bufs, x, fmt, M, s, hist, m0, scale, in_off=0, want_hist_out=True):
    """one call at the test's offsets: rows [M, n_out] complex64 and hist_out (the format's dtype, [23 M, 2]); checks every
    byte of the output allocation outside the rows, and the bytes behind hist_out"""
    bps, n_out = BPS[fmt], len(x) // M
    stride = n_out + 5
    bufs["inp"].upload(np.concatenate([np.full(in_off * bps, 0x5A, np.uint8), bits_of(x), np.full(16, 0x5A, np.uint8)]))
    if hist is not None:
        bufs["hist"].upload(bits_of(hist))
    fill(bufs["out"])
    fill(bufs["hout"])
    out_ptr = bufs["out"].ptr + 24                            # 8 bytes past a 16-byte boundary
    assert bufs["out"].ptr % 16 == 0
    rx.channelize_dev(bufs["inp"].ptr + in_off * bps, fmt, n_out, M, s, out_ptr, stride, hist_ptr=None if hist is None else bufs["hist"].ptr,
                      hist_out_ptr=bufs["hout"].ptr if want_hist_out else None, m0=m0, scale=scale_of(fmt, scale))
    raw = download_fenced(bufs["out"], [(24 + k * stride * 8, n_out * 8) for k in range(M)], "its rows")
    rows = np.stack([raw[24 + k * stride * 8:][:n_out * 8].view(np.complex64) for k in range(M)])
    nh = 23 * M * bps if want_hist_out else 0
    hraw = download_fenced(bufs["hout"], [(0, nh)], "hist_out")
    dt = np.float32 if fmt == cr.FC32 else cr.DTYPE[fmt]
    return rows, hraw[:nh].view(dt).reshape(-1, 2)


@pytest.mark.parametrize("M,s,fmt", CASES)
def test_sizes_offsets_hist_and_m0(rx, bufs, M, s, fmt):
    rng = np.random.default_rng(1000 * M + 10 * s + fmt)
    for n_out in SIZES:
        x = samples(rng, n_out * M, fmt)
        h = samples(rng, 23 * M, fmt)
        for in_off, with_hist, m0, scale in COMBOS:
            hist = h if with_hist else None
            got, hout = run_dev(rx, bufs, x, fmt, M, s, hist, m0, scale, in_off)
            want = zr.analyse_format(x, fmt, scale_of(fmt, scale), M, s, hist, m0)
            assert same_bits(got, want), (n_out, in_off, with_hist, m0)
            assert same_bits(hout, zr.next_history(x, hist, M)), (n_out, in_off, with_hist)


@pytest.mark.parametrize("M,s,fmt", CASES)
def test_a_stream_cut_into_calls_is_the_uncut_stream(rx, bufs, M, s, fmt):
    """hist_out of a call as the next call's hist, m0 advanced by its outputs: byte-identical from output 0 -- one stream in
    three calls cut at 1 and 24 outputs, and in two cut at T + 1"""
    rng = np.random.default_rng(77 * M + s + 3 * fmt)
    n_out, m0 = 2 * T + 3, 11
    x = samples(rng, n_out * M, fmt)
    whole, hist_end = run_dev(rx, bufs, x, fmt, M, s, None, m0, None)
    assert same_bits(whole, zr.analyse_format(x, fmt, scale_of(fmt, None), M, s, None, m0))
    for cuts in ((1, 24), (T + 1,)):
        hist, parts, pos = None, [], 0
        for end in cuts + (n_out,):
            y, hist = run_dev(rx, bufs, x[pos * M:end * M], fmt, M, s, hist, m0 + pos, None)
            parts.append(y)
            pos = end
        assert same_bits(np.concatenate(parts, axis=1), whole), cuts
        assert same_bits(hist, hist_end), cuts


def test_hist_out_on_the_device_feeds_the_next_call(rx, bufs):
    """the same through device pointers alone: hist_out of call one is hist of call two, in the second of two buffers"""
    M, s, fmt, n1, n2 = 4, 1, cr.SC16, 40, 50
    x = samples(np.random.default_rng(5), (n1 + n2) * M, fmt)
    d_in, d_out = bufs["inp"], bufs["out"]
    d_in.upload(bits_of(x))
    rx.channelize_dev(d_in.ptr, fmt, n1, M, s, d_out.ptr, n1 + n2, hist_out_ptr=bufs["hout"].ptr, m0=0)
    rx.channelize_dev(d_in.ptr + n1 * M * 4, fmt, n2, M, s, d_out.ptr + n1 * 8, n1 + n2, hist_ptr=bufs["hout"].ptr,
                      hist_out_ptr=bufs["hout2"].ptr, m0=n1)
    got = d_out.download(np.complex64, M * (n1 + n2)).reshape(M, -1)
    assert same_bits(got, zr.analyse_format(x, fmt, cr.SCALE[fmt], M, s))
    assert same_bits(bufs["hout2"].download(np.int16, 23 * M * 2).reshape(-1, 2), x[-23 * M:])


def test_no_outputs_still_hands_on_the_history(rx, bufs):
    M, fmt = 8, cr.SC8
    h = samples(np.random.default_rng(6), 23 * M, fmt)
    got, hout = run_dev(rx, bufs, h[:0], fmt, M, 1, h, 3, None)
    assert got.shape == (M, 0) and same_bits(hout, h)
    got, hout = run_dev(rx, bufs, h[:0], fmt, M, 1, None, 3, None)
    assert same_bits(hout, np.zeros_like(h))
    # and with neither outputs nor hist_out, NULL in and out are taken
    assert capi.lib().wifirx_channelize(rx._h, None, fmt, 1.0, None, None, M, 1, 0, 0, None, 0) == capi.OK


def test_hist_out_of_a_call_one_block_short_of_the_history(rx, bufs):
    """M = 2, sc16: the call's input is whole blocks of M samples, and SIZES has 0, 1, 23, 24 and 25 of them -- none, one, and
    the history's 23 with one more and two more.  The one that is missing, 22: hist_out is hist's last block (zeros for a
    NULL hist), then the whole input."""
    M, fmt, H = 2, cr.SC16, 23 * 2
    rng = np.random.default_rng(9)
    x, h = samples(rng, 22 * M, fmt), samples(rng, H, fmt)
    for hist in (None, h):
        _, hout = run_dev(rx, bufs, x, fmt, M, 1, hist, 0, None)
        assert same_bits(hout, np.concatenate([np.zeros_like(h) if hist is None else h, x])[-H:]), hist is None


def test_one_large_call(rx):
    """2^20 outputs per channel at M = 8, sc8: 4096 sampled outputs per channel, the last ones included"""
    M, s, fmt, n_out = 8, 1, cr.SC8, 1 << 20
    rng = np.random.default_rng(8)
    x = rng.integers(-128, 128, (n_out * M, 2), dtype=np.int8)
    pick = np.unique(np.concatenate([rng.integers(0, n_out, 4096 - 64), np.arange(32), np.arange(n_out - 32, n_out)]))
    d_in, d_out = rx.alloc(x.nbytes), rx.alloc(M * n_out * 8)
    try:
        d_in.upload(x)
        rx.channelize_dev(d_in.ptr, fmt, n_out, M, s, d_out.ptr, n_out, m0=1)
        got = d_out.download(np.complex64, M * n_out).reshape(M, n_out)[:, pick]
    finally:
        d_in.free()
        d_out.free()
    want = zr.analyse_format(x, fmt, cr.SCALE[fmt], M, s, None, 1, outputs=pick)
    assert same_bits(got, want)


def test_refused_arguments_leave_every_buffer_alone(rx, bufs):
    lib, h, n = capi.lib(), rx._h, 64
    nan, inf = float("nan"), float("inf")
    i, hi, ho, o = bufs["inp"].ptr, bufs["hist"].ptr, bufs["hout"].ptr, bufs["out"].ptr
    big = rx.alloc(1 << 16)
    b = big.ptr
    # (in, fmt, scale, hist, hist_out, n_channels, stacking, n_out, m0, out, out_stride)
    einval = [
        (None, 0, 1.0, hi, ho, 4, 1, n, 0, o, n), (i, 0, 1.0, hi, ho, 4, 1, n, 0, None, n),
        (i, 3, 1.0, hi, ho, 4, 1, n, 0, o, n), (i, -1, 1.0, hi, ho, 4, 1, n, 0, o, n),
        (i, 1, 0.0, hi, ho, 4, 1, n, 0, o, n), (i, 2, -1.0, hi, ho, 4, 1, n, 0, o, n), (i, 1, nan, hi, ho, 4, 1, n, 0, o, n),
        (i, 2, inf, hi, ho, 4, 1, n, 0, o, n),
        (i, 0, 1.0, hi, ho, 0, 1, n, 0, o, n), (i, 0, 1.0, hi, ho, 1, 1, n, 0, o, n), (i, 0, 1.0, hi, ho, 3, 1, n, 0, o, n),
        (i, 0, 1.0, hi, ho, 16, 1, n, 0, o, n),
        (i, 0, 1.0, hi, ho, 4, 2, n, 0, o, n), (i, 0, 1.0, hi, ho, 4, -1, n, 0, o, n),
        (i + 4, 0, 1.0, hi, ho, 4, 1, n, 0, o, n), (i + 2, 1, 1.0, hi, ho, 4, 1, n, 0, o, n), (i + 1, 2, 1.0, hi, ho, 4, 1, n, 0, o, n),
        (i, 0, 1.0, hi + 4, ho, 4, 1, n, 0, o, n), (i, 1, 1.0, hi, ho + 2, 4, 1, n, 0, o, n), (i, 0, 1.0, hi, ho, 4, 1, n, 0, o + 4, n),
        # overlaps: in / out, hist / out, hist_out / out, hist_out / in, hist_out / hist, hist / in; the last row's end counts
        (b, 0, 1.0, None, None, 4, 1, n, 0, b, n), (b + 3 * (n + 1) * 8 + n * 8 - 8, 0, 1.0, None, None, 4, 1, n, 0, b, n + 1),
        (i, 0, 1.0, b, None, 4, 1, n, 0, b + 8, n), (i, 0, 1.0, None, b + 4 * n * 8 - 8, 4, 1, n, 0, b, n),
        (b, 0, 1.0, None, b + 4 * n * 8 - 8, 4, 1, n, 0, o, n), (i, 0, 1.0, b, b + 23 * 4 * 8 - 8, 4, 1, n, 0, o, n),
        (b + 23 * 4 * 2 - 2, 2, 1.0, b, None, 4, 1, n, 0, o, n), (i, 0, 1.0, hi, hi, 4, 1, n, 0, o, n),
    ]
    erange = [
        (i, 0, 1.0, hi, ho, 4, 1, n, 0, o, n - 1), (i, 0, 1.0, hi, ho, 4, 1, n, 0, o, 0),
        (i, 0, 1.0, hi, ho, 4, 1, (1 << 40) + 1, 0, o, 1 << 41), (i, 0, 1.0, hi, ho, 8, 1, 1 << 62, 0, o, 1 << 62),
        (i, 0, 1.0, hi, ho, 8, 1, (1 << 64) - 1, 0, o, (1 << 64) - 1),
    ]
    try:
        fills = {k: fill(d) for k, d in bufs.items()}
        fill(big)
        for a in einval:
            assert lib.wifirx_channelize(h, *a) == capi.EINVAL, a
        for a in erange:
            assert lib.wifirx_channelize(h, *a) == capi.ERANGE, a
        rx.sync()
        for k, d in bufs.items():
            assert np.array_equal(d.download(np.uint8, d.nbytes), fills[k]), k
        assert (big.download(np.uint8, 1 << 16) == CANARY).all()
        # buffers that only touch are taken: hist, in, hist_out and out one behind the other
        n_h = 23 * 4 * 8
        assert lib.wifirx_channelize(h, b + n_h, 0, 1.0, b, b + n_h + 4 * n * 8, 4, 1, n, 0, b + 2 * n_h + 4 * n * 8, n) == capi.OK
        rx.sync()
    finally:
        big.free()
