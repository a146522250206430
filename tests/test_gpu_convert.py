"""wifirx_iq_to_f32 / wifirx_iq_from_f32 (wr_convert.hip) against tests/convert_ref.py, bit for bit: every size around the
kernels' 16-byte pieces, both peeled heads, every integer value, the special values, the clip count, the refused arguments --
and the loop-back with the converter between channel and receiver against the oracle on host-quantised samples."""
import ctypes as C
import math

import numpy as np
import pytest

import convert_ref as cr
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 4099)
OFFSETS = ((0, 0), (0, 1), (1, 0), (1, 1))              # (source, destination) start, in samples into their allocations
SCALES = (2.0 ** -15, 2.0 ** -7, 1.0 / 3.0)
CANARY = 0xA5
ROOM = 4099 + 1 + 8                                     # samples per scratch allocation: the largest case, its offset, a margin
BPS = {cr.SC16: 4, cr.SC8: 2}


@pytest.fixture(scope="module")
def rx():
    r = capi.WifiRx(max_sym=1, device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def bufs(rx):
    """one integer-side and one float-side scratch allocation for the small cases"""
    b = rx.alloc(ROOM * 4), rx.alloc(ROOM * 8)
    yield b
    for d in b:
        d.free()


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint8)


def widen_dev(rx, bufs, q, fmt, scale, s_off, d_off):
    """q [n, 2] through wifirx_iq_to_f32 at the two offsets; returns the float32 pairs [n, 2]; checks the bytes around them"""
    d_int, d_flt = bufs
    n, bps = len(q), BPS[fmt]
    d_int.upload(np.concatenate([np.zeros(s_off * bps, np.uint8), bits_of(q).reshape(-1)]))
    d_flt.upload(np.full(ROOM * 8, CANARY, np.uint8))
    rx.iq_to_f32_dev(d_int.ptr + s_off * bps, fmt, n, d_flt.ptr + d_off * 8, scale)
    out = d_flt.download(np.uint8, ROOM * 8)
    assert (out[:d_off * 8] == CANARY).all() and (out[(d_off + n) * 8:] == CANARY).all(), "wrote outside its destination"
    return out[d_off * 8:(d_off + n) * 8].view(np.float32).reshape(-1, 2)


def quantise_dev(rx, bufs, x, fmt, scale, bits, s_off, d_off, count=True):
    """x float32 [n, 2] through wifirx_iq_from_f32; returns (integers [n, 2], clipped or None)"""
    d_int, d_flt = bufs
    n, bps = len(x), BPS[fmt]
    d_flt.upload(np.concatenate([np.zeros(s_off * 8, np.uint8), bits_of(x).reshape(-1)]))
    d_int.upload(np.full(ROOM * 4, CANARY, np.uint8))
    clipped = rx.iq_from_f32_dev(d_flt.ptr + s_off * 8, n, fmt, d_int.ptr + d_off * bps, scale, bits, count=count)
    out = d_int.download(np.uint8, ROOM * 4)
    assert (out[:d_off * bps] == CANARY).all() and (out[(d_off + n) * bps:] == CANARY).all(), "wrote outside its destination"
    return out[d_off * bps:(d_off + n) * bps].view(cr.DTYPE[fmt]).reshape(-1, 2), clipped


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8])
def test_widen_sizes_and_heads(rx, bufs, fmt, scale):
    rng = np.random.default_rng(fmt)
    info = np.iinfo(cr.DTYPE[fmt])
    for n in SIZES:
        q = rng.integers(info.min, info.max + 1, (n, 2)).astype(cr.DTYPE[fmt])
        want = cr.widen(q, scale)
        for s_off, d_off in OFFSETS:
            got = widen_dev(rx, bufs, q, fmt, scale, s_off, d_off)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, s_off, d_off)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8])
def test_widen_every_integer_value(rx, fmt, scale):
    if fmt == cr.SC16:      # every int16 value in I against the reversed order in Q
        v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
        q = np.stack([v, v[::-1]], axis=1)
    else:                   # all 256 x 256 int8 pairs
        v = np.arange(-128, 128, dtype=np.int32).astype(np.int8)
        q = np.stack([np.repeat(v, 256), np.tile(v, 256)], axis=1)
    got = rx.iq_to_f32(q, scale=scale)
    want = cr.widen(q, scale)
    assert np.array_equal(got.view(np.uint32).reshape(-1, 2), want.view(np.uint32))
    if scale != SCALES[2]:
        assert np.array_equal(got.view(np.float32).astype(np.float64).reshape(-1, 2), q.astype(np.float64) * scale)      # exact


@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8])
def test_quantise_sizes_and_heads(rx, bufs, fmt):
    rng = np.random.default_rng(10 + fmt)
    bits = cr.MAX_BITS[fmt]
    scale = np.float32(2.0 ** (bits - 1) / 2.5)        # about 1 % of the components clip
    for n in SIZES:
        x = rng.standard_normal((n, 2)).astype(np.float32)
        want, want_clipped = cr.quantise(x, scale, fmt)
        for s_off, d_off in OFFSETS:
            got, clipped = quantise_dev(rx, bufs, x, fmt, scale, bits, s_off, d_off)
            assert np.array_equal(got, want) and clipped == want_clipped, (n, s_off, d_off)


@pytest.mark.parametrize("fmt,bits", [(cr.SC16, 16), (cr.SC16, 5), (cr.SC8, 8), (cr.SC8, 2)])
def test_quantise_special_values(rx, bufs, fmt, bits):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    hi, lo = 2 ** (bits - 1) - 1, -(2 ** (bits - 1))
    row = np.array([nan, 1.0, inf, -inf, 0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, hi, hi + 0.5, hi + 1, lo, lo - 0.5, lo - 1,
                    3e38, -3e38, 1e-40, -nan], np.float32)
    x = np.resize(row, 2 * 71).reshape(-1, 2)            # 71 samples: whole pieces and an edge, the values at every position
    for scale in (1.0, 4.0):
        want, want_clipped = cr.quantise(x, scale, fmt, bits)
        assert want_clipped > 0
        for s_off, d_off in OFFSETS:
            got, clipped = quantise_dev(rx, bufs, x, fmt, scale, bits, s_off, d_off)
            assert np.array_equal(got, want) and clipped == want_clipped, (scale, s_off, d_off)


@pytest.mark.parametrize("fmt,bits", [(cr.SC16, 4), (cr.SC16, 8), (cr.SC16, 12), (cr.SC16, 16), (cr.SC8, 4), (cr.SC8, 8)])
def test_quantise_gaussian_and_the_clip_count(rx, fmt, bits):
    x = np.random.default_rng(bits).standard_normal((1 << 16, 2)).astype(np.float32)
    scale = np.float32(2.0 ** (bits - 1) / 2.576)      # full scale at the two-sided 1 % point
    want, want_clipped = cr.quantise(x, scale, fmt, bits)
    assert 0.005 < want_clipped / x.size < 0.02
    got, clipped = rx.iq_from_f32(cr.to_complex(x), fmt, scale=scale, bits=bits)
    assert np.array_equal(got, want) and clipped == want_clipped


def test_without_a_counter_nothing_is_counted(rx, bufs):
    """clipped = NULL: the same integers; and the handle's counter is not an accumulator -- a counted call before and after
    one without a counter returns its own count both times"""
    x = np.random.default_rng(5).standard_normal((4099, 2)).astype(np.float32)
    scale = np.float32(127 / 2.0)
    want, want_clipped = cr.quantise(x, scale, cr.SC8)
    assert want_clipped > 100
    got, clipped = quantise_dev(rx, bufs, x, cr.SC8, scale, 8, 0, 0)
    assert clipped == want_clipped and np.array_equal(got, want)
    got, clipped = quantise_dev(rx, bufs, x, cr.SC8, scale, 8, 0, 0, count=False)
    assert clipped is None and np.array_equal(got, want)
    got, clipped = quantise_dev(rx, bufs, x[:100], cr.SC8, scale, 8, 0, 0)
    assert clipped == cr.quantise(x[:100], scale, cr.SC8)[1]
    # n = 0 with a counter: zero, nothing queued
    c = C.c_uint64(77)
    assert capi.lib().wifirx_iq_from_f32(rx._h, bufs[1].ptr, 0, 1.0, cr.SC8, 8, bufs[0].ptr, C.byref(c)) == capi.OK and c.value == 0


def test_refused_arguments_leave_the_destination_alone(rx, bufs):
    d_int, d_flt = bufs
    lib, h, n = capi.lib(), rx._h, 64
    nan, inf = float("nan"), float("inf")
    big = rx.alloc(4096)
    try:
        to_f32 = [                                             # (src, fmt, n, scale, dst)
            (None, cr.SC16, n, 1.0, d_flt.ptr), (d_int.ptr, cr.SC16, n, 1.0, None),
            (d_int.ptr, cr.FC32, n, 1.0, d_flt.ptr), (d_int.ptr, 3, n, 1.0, d_flt.ptr), (d_int.ptr, -1, n, 1.0, d_flt.ptr),
            (d_int.ptr, cr.SC16, n, 0.0, d_flt.ptr), (d_int.ptr, cr.SC8, n, -1.0, d_flt.ptr), (d_int.ptr, cr.SC16, n, nan, d_flt.ptr),
            (d_int.ptr, cr.SC8, n, inf, d_flt.ptr),
            (d_int.ptr + 2, cr.SC16, n, 1.0, d_flt.ptr), (d_int.ptr + 1, cr.SC8, n, 1.0, d_flt.ptr), (d_int.ptr, cr.SC16, n, 1.0, d_flt.ptr + 4),
            (big.ptr, cr.SC16, n, 1.0, big.ptr), (big.ptr + n * 4 - 8, cr.SC16, n, 1.0, big.ptr + n * 4 - 8 + 8),      # overlaps
            (big.ptr + n * 8 - 2, cr.SC8, n, 1.0, big.ptr), (big.ptr + 1024, cr.SC8, n, 1.0, big.ptr + 1024 - n * 8 + 8),
        ]
        from_f32 = [                                           # (src, n, scale, fmt, bits, dst)
            (None, n, 1.0, cr.SC16, 16, d_int.ptr), (d_flt.ptr, n, 1.0, cr.SC16, 16, None),
            (d_flt.ptr, n, 1.0, cr.FC32, 16, d_int.ptr), (d_flt.ptr, n, 1.0, 3, 8, d_int.ptr),
            (d_flt.ptr, n, 0.0, cr.SC16, 16, d_int.ptr), (d_flt.ptr, n, -2.0, cr.SC8, 8, d_int.ptr), (d_flt.ptr, n, nan, cr.SC16, 16, d_int.ptr),
            (d_flt.ptr, n, inf, cr.SC8, 8, d_int.ptr),
            (d_flt.ptr, n, 1.0, cr.SC16, 1, d_int.ptr), (d_flt.ptr, n, 1.0, cr.SC16, 17, d_int.ptr), (d_flt.ptr, n, 1.0, cr.SC8, 9, d_int.ptr),
            (d_flt.ptr, n, 1.0, cr.SC8, 0, d_int.ptr),
            (d_flt.ptr + 4, n, 1.0, cr.SC16, 16, d_int.ptr), (d_flt.ptr, n, 1.0, cr.SC16, 16, d_int.ptr + 2), (d_flt.ptr, n, 1.0, cr.SC8, 8, d_int.ptr + 1),
            (big.ptr, n, 1.0, cr.SC16, 16, big.ptr), (big.ptr, n, 1.0, cr.SC8, 8, big.ptr + n * 8 - 2),               # overlaps
            (big.ptr + 1024, n, 1.0, cr.SC16, 16, big.ptr + 1024 - n * 4 + 4),
        ]
        canary_f, canary_i, canary_b = np.full(ROOM * 8, CANARY, np.uint8), np.full(ROOM * 4, CANARY, np.uint8), np.full(4096, CANARY, np.uint8)
        d_flt.upload(canary_f)
        d_int.upload(canary_i)
        big.upload(canary_b)
        clipped = C.c_uint64(123)
        for a in to_f32:
            assert lib.wifirx_iq_to_f32(h, a[0], a[1], a[2], a[3], a[4]) == capi.EINVAL, a
        for a in from_f32:
            assert lib.wifirx_iq_from_f32(h, a[0], a[1], a[2], a[3], a[4], a[5], C.byref(clipped)) == capi.EINVAL, a
            assert lib.wifirx_iq_from_f32(h, a[0], a[1], a[2], a[3], a[4], a[5], None) == capi.EINVAL, a
        assert clipped.value == 123
        rx.sync()
        assert np.array_equal(d_flt.download(np.uint8, ROOM * 8), canary_f) and np.array_equal(d_int.download(np.uint8, ROOM * 4), canary_i)
        assert np.array_equal(big.download(np.uint8, 4096), canary_b)
        # buffers that only touch are taken: the integers right behind / in front of the floats
        assert lib.wifirx_iq_to_f32(h, big.ptr + n * 8, cr.SC16, n, 1.0, big.ptr) == capi.OK
        assert lib.wifirx_iq_from_f32(h, big.ptr + n * 2, n, 1.0, cr.SC8, 8, big.ptr, None) == capi.OK
        rx.sync()
    finally:
        big.free()


def test_loop_back_with_the_converter_equals_the_oracle_on_host_quantised_samples(orc):
    """TX -> channel -> quantise (sc8, 8 bits, full scale 12 dB above the RMS of the channel output) -> widen -> demod ->
    decode_mac on the device; the same samples quantised and widened by convert_ref and run through the oracle"""
    n, enc, plen, lead, slot = 48, 7, 294, 160, 1472
    n_sym = txgen.n_sym_for(plen, enc)
    rx = capi.WifiRx(max_sym=n_sym, chan_est=capi.EQ_LS, device=0)
    d_psdu, rows, iq, d_q, iq2 = rx.alloc(n * plen), rx.alloc(n * slot * 8), rx.alloc(n * slot * 8), rx.alloc(n * slot * 2), rx.alloc(n * slot * 8)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    try:
        rx.mac_batch_dev(d_psdu.ptr, plen, n, None, payload_len=plen - 28, payload_seed=4)
        rx.tx_batch_dev(rows.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=lead, row_len=slot)
        cfo = np.random.default_rng(8).uniform(-0.037, 0.037, n).astype(np.float32)
        rx.channel_dev(rows.ptr, iq.ptr, n * slot, n, row_len=slot, taps=(1.0, 0.2 - 0.1j), cfo=cfo, gain=math.sqrt(10 ** (32 / 10)), noise_voltage=1.0, seed=21)
        y = iq.download(np.complex64, n * slot)
        scale_q = cr.full_scale(y, 12.0, cr.SC8)
        scale_w = np.float32(1.0 / float(scale_q))
        clipped = rx.iq_from_f32_dev(iq.ptr, n * slot, cr.SC8, d_q.ptr, scale_q, 8, count=True)
        rx.iq_to_f32_dev(d_q.ptr, cr.SC8, n * slot, iq2.ptr, scale_w)
        rx.demod_batch_dev(iq2.ptr, slot, n, dev)
        rx.decode_batch_dev(n, dev)
        rx.sync()
        got = rx.download_out(dev, n)
        q_dev = d_q.download(np.int8, 2 * n * slot).reshape(-1, 2)
    finally:
        rx.free_out(dev)
        for b in (d_psdu, rows, iq, d_q, iq2):
            b.free()
        rx.close()
    q, want_clipped = cr.quantise(cr.pairs(y), scale_q, cr.SC8)
    assert np.array_equal(q_dev, q) and clipped == want_clipped
    prm = orc.make_params(max_sym=n_sym)
    o = orc.demod_batch(cr.to_complex(cr.widen(q, scale_w)), slot, prm)
    opsdu = orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=304)
    assert np.array_equal(got["frames"], o["frames"]) and np.array_equal(got["idx"], o["idx"])
    ok = (got["frames"]["flags"] & capi.F_CRC_OK) != 0
    assert ok.sum() >= n // 2, "the converter's operating point lost the link: the comparison would be of failures"
    for k in range(n):
        if got["frames"]["flags"][k] & capi.F_DECODED:
            assert np.array_equal(got["psdu"][k, :plen], opsdu[k, :plen]), k
