"""wifirx_combine (wr_combiner.hip) against tests/combine_ref.py, bit for bit: every size around the 24-tap window and the
kernel's tile, every channel count and stacking, hist and hist_out, both parities of m0, rows wider than their samples,
gains, buffers at 8 but not 16 bytes, out and hist_out between fences, a stream cut into calls, the block, and the refused
arguments."""
import ctypes as C

import numpy as np
import pytest

import combine_ref as cb
from bank_helpers import CANARY, alloc_bufs, bits_of, download_fenced, fill, open_rx, same_bits, tile
from wifirx import block, capi

pytestmark = pytest.mark.gpu

T = tile("wr_combiner.h", "WR_CB_TILE")
assert T == 512
SIZES = (1, 2, 23, 24, 25, T - 1, T, T + 1, 2 * T + 1, 3 * T + 7)
N_MAX = max(SIZES)
FENCE = 4096
CASES = [pytest.param(M, s, id="M%d-s%d" % (M, s)) for M in (2, 4, 8) for s in (0, 1)]
# (hist given, m0, in_stride - n_in, gains given, input offset in bytes, output offset in bytes)
COMBOS = ((False, 0, 0, False, 0, 0), (True, 7, 3, True, 8, 8), (True, 1 << 40, 4, False, 8, 0), (False, 11, 1, True, 0, 8))
IN_ROOM = 16 + 8 * (N_MAX + 4) * 8 + 16
OUT_ROOM = FENCE + 16 + N_MAX * 8 * 8 + FENCE
HIST_ROOM = FENCE + 23 * 8 * 8 + FENCE


@pytest.fixture(scope="module")
def rx():
    yield from open_rx()


@pytest.fixture(scope="module")
def bufs(rx):
    yield from alloc_bufs(rx, inp=IN_ROOM, hist=23 * 8 * 8, hout=HIST_ROOM, hout2=HIST_ROOM, out=OUT_ROOM)


def streams(rng, M, n):
    return (rng.standard_normal((M, n)) + 1j * rng.standard_normal((M, n))).astype(np.complex64)


def gains_of(M):
    """one gain 0, one negative"""
    g = (0.5 + 0.375 * np.arange(M)).astype(np.float32)
    g[0], g[M - 1] = -0.75, 0.0
    return g


def run_dev(rx, bufs, u, M, s, hist=None, m0=0, extra=0, gains=None, in_off=0, out_off=0, hout="hout", want_hist_out=True):
    """one call: (wide stream complex64 [n M], hist_out complex64 [M, 23]); the rows lie `extra` samples apart in a buffer of
    NaNs; checks the fences around out and hist_out"""
    n = u.shape[1]
    stride = n + extra
    raw = np.full(IN_ROOM, 0xFF, np.uint8)                   # NaNs wherever no sample lies
    for k in range(M):
        a = in_off + k * stride * 8
        raw[a:a + n * 8] = bits_of(u[k])
    bufs["inp"].upload(raw)
    if hist is not None:
        bufs["hist"].upload(bits_of(hist))
    fill(bufs["out"])
    fill(bufs[hout])
    assert bufs["out"].ptr % 16 == 0 and bufs["inp"].ptr % 16 == 0
    rx.combine_dev(bufs["inp"].ptr + in_off, stride, n, M, s, bufs["out"].ptr + FENCE + out_off, gains=gains,
                   hist_ptr=None if hist is None else bufs["hist"].ptr,
                   hist_out_ptr=bufs[hout].ptr + FENCE if want_hist_out else None, m0=m0)
    a = FENCE + out_off
    got = download_fenced(bufs["out"], [(a, n * M * 8)], "out")
    nh = 23 * M * 8 if want_hist_out else 0
    hraw = download_fenced(bufs[hout], [(FENCE, nh)], "hist_out")
    return got[a:a + n * M * 8].view(np.complex64), hraw[FENCE:FENCE + nh].view(np.complex64).reshape(-1, 23)


@pytest.mark.parametrize("M,s", CASES)
def test_sizes_hist_m0_stride_gains_and_alignment(rx, bufs, M, s):
    rng = np.random.default_rng(1000 * M + s)
    for n in SIZES:
        u, h = streams(rng, M, n), streams(rng, M, 23)
        for with_hist, m0, extra, with_gains, in_off, out_off in COMBOS:
            hist, g = h if with_hist else None, gains_of(M) if with_gains else None
            got, hout = run_dev(rx, bufs, u, M, s, hist, m0, extra, g, in_off, out_off)
            assert same_bits(got, cb.combine(u, M, s, g, hist, m0)), (n, with_hist, m0, extra, with_gains, in_off, out_off)
            assert same_bits(hout, cb.next_history(u, hist, M)), (n, with_hist)


@pytest.mark.parametrize("M,s", CASES)
def test_a_stream_cut_into_three_uneven_calls_is_the_uncut_stream(rx, bufs, M, s):
    """hist_out of a call is the next call's hist, in two buffers used in turn, m0 advanced by the samples taken"""
    rng = np.random.default_rng(77 * M + s)
    n, m0, g = 2 * T + 3, 11, gains_of(M)
    u = streams(rng, M, n)
    whole, hist_end = run_dev(rx, bufs, u, M, s, None, m0, 0, g)
    assert same_bits(whole, cb.combine(u, M, s, g, None, m0))
    for cuts in ((1, 24), (T + 1, T + 24)):
        hist, parts, pos = None, [], 0
        for i, end in enumerate(cuts + (n,)):
            y, hist = run_dev(rx, bufs, u[:, pos:end], M, s, hist, m0 + pos, 0, g, hout=("hout", "hout2")[i & 1])
            parts.append(y)
            pos = end
        assert same_bits(np.concatenate(parts), whole), cuts
        assert same_bits(hist, hist_end), cuts


def test_hist_out_on_the_device_feeds_the_next_call(rx, bufs):
    """the same through device pointers alone: hist_out of call one is hist of call two, in the second of two buffers"""
    M, s, n1, n2 = 4, 1, 40, 51
    u = streams(np.random.default_rng(5), M, n1 + n2)
    d_in, d_out = bufs["inp"], bufs["out"]
    d_in.upload(u)
    rx.combine_dev(d_in.ptr, n1 + n2, n1, M, s, d_out.ptr, hist_out_ptr=bufs["hout"].ptr, m0=0)
    rx.combine_dev(d_in.ptr + n1 * 8, n1 + n2, n2, M, s, d_out.ptr + n1 * M * 8, hist_ptr=bufs["hout"].ptr,
                   hist_out_ptr=bufs["hout2"].ptr, m0=n1)
    assert same_bits(d_out.download(np.complex64, M * (n1 + n2)), cb.combine(u, M, s))
    assert same_bits(bufs["hout2"].download(np.complex64, 23 * M).reshape(M, 23), u[:, -23:])


def test_no_samples_still_hand_on_the_history(rx, bufs):
    M = 8
    h = streams(np.random.default_rng(6), M, 23)
    got, hout = run_dev(rx, bufs, h[:, :0], M, 1, h, 3)
    assert got.shape == (0,) and same_bits(hout, h)
    got, hout = run_dev(rx, bufs, h[:, :0], M, 1, None, 3)
    assert same_bits(hout, np.zeros_like(h))
    # and with neither samples nor hist_out, NULL in and out are taken
    assert capi.lib().wifirx_combine(rx._h, None, 0, None, None, None, M, 1, 0, 0, None) == capi.OK


def test_host_array_convenience(rx):
    u = streams(np.random.default_rng(7), 4, 100)
    g = gains_of(4)
    assert same_bits(rx.combine(u, 1, g), cb.combine(u, 4, 1, g))


def test_block_in_uneven_work_chunks_is_one_call():
    M, s, n, g = 4, 1, T + 300, gains_of(4)
    u = streams(np.random.default_rng(8), M, n)
    want = cb.combine(u, M, s, g)
    blk = block.wideband_combiner(M, s, gains=g)
    try:
        assert blk.in_sig == [np.complex64] * M and blk.out_sig == [np.complex64]
        out, pos = [], 0
        # (items offered per input, room in the output): the room bounds one call, the shortest input another
        for offered, room in ((1, 64), (30, M * 22 + 3), (T, 8 * T), (n, 8 * n), (n, 8 * n)):
            if pos == n:
                break
            ins = [u[k, pos:pos + offered + (k & 1)] for k in range(M)]
            o = np.full(room, np.nan, np.complex64)
            made = blk.work(ins, [o])
            took = min(offered, n - pos, room // M)
            assert made == took * M and not np.isnan(o[:made]).any() and np.isnan(o[made:]).all()
            out.append(o[:made])
            pos += took
        assert pos == n and same_bits(np.concatenate(out), want)
        blk.set_gains(None)
        with pytest.raises(ValueError):
            blk.set_gains([1.0, float("nan"), 1.0, 1.0])
    finally:
        blk.close()


def test_refused_arguments_leave_every_buffer_alone(rx, bufs):
    lib, h, n = capi.lib(), rx._h, 64
    i, hi, ho, o = bufs["inp"].ptr, bufs["hist"].ptr, bufs["hout"].ptr, bufs["out"].ptr
    big = rx.alloc(1 << 16)
    b = big.ptr
    F4 = C.c_float * 4
    ok, nan, inf = F4(1, 1, 1, 1), F4(1, float("nan"), 1, 1), F4(1, 1, 1, float("-inf"))
    n_h = 23 * 4 * 8
    # (in, in_stride, gains, hist, hist_out, n_channels, stacking, n_in, m0, out)
    einval = [
        (None, n, ok, hi, ho, 4, 1, n, 0, o), (i, n, ok, hi, ho, 4, 1, n, 0, None),
        (i, n, ok, hi, ho, 0, 1, n, 0, o), (i, n, ok, hi, ho, 1, 1, n, 0, o), (i, n, ok, hi, ho, 3, 1, n, 0, o),
        (i, n, None, hi, ho, 16, 1, n, 0, o),
        (i, n, ok, hi, ho, 4, 2, n, 0, o), (i, n, ok, hi, ho, 4, -1, n, 0, o),
        (i, n, nan, hi, ho, 4, 1, n, 0, o), (i, n, inf, hi, ho, 4, 1, n, 0, o),
        (i + 4, n, ok, hi, ho, 4, 1, n, 0, o), (i, n, ok, hi + 4, ho, 4, 1, n, 0, o), (i, n, ok, hi, ho + 2, 4, 1, n, 0, o),
        (i, n, ok, hi, ho, 4, 1, n, 0, o + 4),
        # overlaps: in / out, the last input row's end / out, hist / out, hist_out / out, hist_out / in, hist_out / hist, hist / in
        (b, n, None, None, None, 4, 1, n, 0, b), (b, n + 1, None, None, None, 4, 1, n, 0, b + 3 * (n + 1) * 8 + n * 8 - 8),
        (i, n, None, b, None, 4, 1, n, 0, b + n_h - 8), (i, n, None, None, b + 4 * n * 8 - 8, 4, 1, n, 0, b),
        (b, n, None, None, b + 4 * n * 8 - 8, 4, 1, n, 0, o), (i, n, None, b, b + n_h - 8, 4, 1, n, 0, o),
        (b + n_h - 8, n, None, b, None, 4, 1, n, 0, o), (i, n, None, hi, hi, 4, 1, n, 0, o),
    ]
    erange = [
        (i, n - 1, ok, hi, ho, 4, 1, n, 0, o), (i, 0, ok, hi, ho, 4, 1, n, 0, o), (i, (1 << 44) + 1, ok, hi, ho, 4, 1, n, 0, o),
        (i, 1 << 41, ok, hi, ho, 4, 1, (1 << 40) + 1, 0, o), (i, (1 << 64) - 1, ok, hi, ho, 8, 1, (1 << 64) - 1, 0, o),
    ]
    try:
        fills = {k: fill(d) for k, d in bufs.items()}
        fill(big)
        for a in einval:
            assert lib.wifirx_combine(h, *a) == capi.EINVAL, a
        for a in erange:
            assert lib.wifirx_combine(h, *a) == capi.ERANGE, a
        rx.sync()
        for k, d in bufs.items():
            assert np.array_equal(d.download(np.uint8, d.nbytes), fills[k]), k
        assert (big.download(np.uint8, 1 << 16) == CANARY).all()
        # buffers that only touch are taken: hist, in, hist_out and out one behind the other
        assert lib.wifirx_combine(h, b + n_h, n, ok, b, b + n_h + 4 * n * 8, 4, 1, n, 0, b + 2 * n_h + 4 * n * 8) == capi.OK
        rx.sync()
    finally:
        big.free()
