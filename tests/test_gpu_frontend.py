"""wifirx_frontend and wifirx_rx_impair (wr_frontend.hip) against tests/frontend_ref.py, byte for byte: the output, the
state, and the bytes around the output."""
import ctypes as C

import numpy as np
import pytest

import frontend_ref as fr

pytestmark = pytest.mark.gpu

B = fr.BLOCK
LENGTHS = [1, 4095, 4096, 4097, 3 * 4096 + 17, 70 * 4096 + 5]
GUARD = 4               # samples of sentinel on either side of the output
SENTINEL = np.float32(-7.25)


@pytest.fixture(scope="module")
def rx():
    from wifirx import capi
    h = capi.WifiRx(max_sym=1)
    yield h
    h.close()


def samples(n, fmt, seed=1):
    """a receiver's samples: noise through an imbalance plus an offset; float pairs carry a NaN and two infinities.
    Returns (the array a caller hands in, scale)"""
    rng = np.random.default_rng(seed + 10 * fmt)
    x = ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.2).astype(np.complex64)
    x = fr.rx_impair(x, *fr.imbalance(1.5, -8.0), 0.11 - 0.07j)
    if fmt == fr.FC32:
        if n > 100:
            x[17], x[50], x[99] = np.nan, np.inf, complex(1e30, -np.inf)
        return x, 1.0
    bits = 16 if fmt == fr.SC16 else 8
    q = np.clip(np.rint(fr.widen(x) * 2.0 ** (bits - 2)), -2 ** (bits - 1), 2 ** (bits - 1) - 1)
    return q.astype(np.int16 if fmt == fr.SC16 else np.int8), 2.0 ** -(bits - 1)


def cfg_of(capi, flags=3, frac_bits=12, dc_shift=2, iq_shift=4):
    return capi.FrontendCfg(flags, frac_bits, dc_shift, iq_shift)


def run_dev(rx, x, fmt, scale, cfg, state=None, out_off=0, in_place=False):
    """one wifirx_frontend call on x: (output complex64 [n], state record); the output starts out_off samples into a buffer
    that is 16-byte aligned, and the sentinels around it must survive"""
    from wifirx import capi
    x = np.ascontiguousarray(x)
    n = x.size if fmt == fr.FC32 else x.size // 2
    st = np.zeros((), capi.FE_STATE_DTYPE) if state is None else np.array(state, dtype=capi.FE_STATE_DTYPE)
    total = out_off + GUARD + n + GUARD
    d_in, d_out, d_st = rx.alloc(max(x.nbytes, 1)), rx.alloc(total * 8), rx.alloc(capi.FE_STATE_DTYPE.itemsize)
    try:
        d_st.upload(st.reshape(1))
        host = np.full(2 * total, SENTINEL, np.float32)
        if in_place:
            host[2 * (out_off + GUARD):2 * (out_off + GUARD + n)] = x.view(np.float32)
        d_out.upload(host)
        d_in.upload(x)
        out_ptr = d_out.ptr + 8 * (out_off + GUARD)
        rx.frontend_dev(cfg, d_st.ptr, out_ptr if in_place else d_in.ptr, fmt, n, out_ptr, scale)
        got = d_out.download(np.float32, 2 * total)
        edge = np.concatenate([got[:2 * (out_off + GUARD)], got[2 * (out_off + GUARD + n):]])
        assert (edge == SENTINEL).all(), "bytes outside the output were written"
        return got[2 * (out_off + GUARD):2 * (out_off + GUARD + n)].copy().view(np.complex64), d_st.download(capi.FE_STATE_DTYPE, 1)[0]
    finally:
        d_in.free()
        d_out.free()
        d_st.free()


def ref(x, fmt, scale, cfg, state=None):
    fe = fr.Frontend(flags=cfg.flags, frac_bits=cfg.frac_bits, dc_shift=cfg.dc_shift, iq_shift=cfg.iq_shift, state=state)
    return fe.process(x, fmt, scale), fe.state()


def same(got, want):
    z, st = got
    wz, wst = want
    # bit for bit, except that a NaN is only required to be a NaN: rule 32 does not say which one an invalid operation gives
    zf, wf = z.view(np.float32), wz.view(np.float32)
    assert np.array_equal(np.isnan(zf), np.isnan(wf)), np.flatnonzero(np.isnan(zf) != np.isnan(wf))[:8]
    diff = (zf.view(np.uint32) != wf.view(np.uint32)) & ~np.isnan(wf)
    assert not diff.any(), np.flatnonzero(diff)[:8]
    assert st.tobytes() == wst.tobytes(), {k: (st[k], wst[k]) for k in ("n", "part", "d0", "w0") if st[k].tobytes() != wst[k].tobytes()}


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("fmt", [fr.FC32, fr.SC16, fr.SC8])
def test_formats_and_lengths(rx, fmt, n):
    """every length around a block, more than the ring, and the output one sample off 16-byte alignment"""
    from wifirx import capi
    x, scale = samples(n, fmt)
    cfg = cfg_of(capi)
    want = ref(x, fmt, scale, cfg)
    for out_off in (0, 1):
        same(run_dev(rx, x, fmt, scale, cfg, out_off=out_off), want)


@pytest.mark.parametrize("n0", [1, 1000, 4095, 4096, 5 * 4096 + 4001])
@pytest.mark.parametrize("fmt", [fr.FC32, fr.SC16, fr.SC8])
def test_a_call_continued_inside_a_block(rx, fmt, n0):
    """the stream origin lies inside a block of the call: a state with an open block (and, for 4096, none)"""
    from wifirx import capi
    x, scale = samples(n0 + 3 * B + 17, fmt, seed=2)
    cfg = cfg_of(capi)
    _, st0 = ref(x[:n0], fmt, scale, cfg)                   # (integer samples are rows of I and Q)
    for n in (1, B - (n0 % B), 3 * B + 17):                 # inside the open block, up to its end, across three more
        want = ref(x[n0:n0 + n], fmt, scale, cfg, state=st0)
        for out_off in (0, 1):
            same(run_dev(rx, x[n0:n0 + n], fmt, scale, cfg, state=st0, out_off=out_off), want)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(12, 2, 4), (0, 0, 6), (30, 6, 0), (12, 6, 6)])
def test_flags_and_settings(rx, flags, shape):
    from wifirx import capi
    x, scale = samples(70 * B + 5, fr.SC16, seed=3)
    cfg = cfg_of(capi, flags, *shape)
    same(run_dev(rx, x, fr.SC16, scale, cfg), ref(x, fr.SC16, scale, cfg))


def test_in_place_for_fc32(rx):
    from wifirx import capi
    cfg = cfg_of(capi)
    for n in (1, 4097, 9 * B + 3):
        x, _ = samples(n, fr.FC32, seed=4)
        for out_off in (0, 1):
            same(run_dev(rx, x, fr.FC32, 1.0, cfg, out_off=out_off, in_place=True), ref(x, fr.FC32, 1.0, cfg))


def test_initial_values(rx):
    from wifirx import capi
    st0 = capi.frontend_state(d0=0.125 - 0.0625j, w0=0.04 - 0.03j)
    x, scale = samples(2 * B + 9, fr.SC8, seed=5)
    for flags in (0, 1, 2, 3):
        cfg = cfg_of(capi, flags)
        got = run_dev(rx, x, fr.SC8, scale, cfg, state=st0)
        same(got, ref(x, fr.SC8, scale, cfg, state=st0))
        assert list(got[1]["d0"]) == [512, -256]


@pytest.mark.parametrize("fmt", [fr.FC32, fr.SC16, fr.SC8])
def test_a_chunked_sequence_equals_one_call(rx, fmt):
    """the state stays on the device between the calls, which are queued without a wait in between"""
    from wifirx import capi
    n = 20 * B + 77
    x, scale = samples(n, fmt, seed=6)
    bps = {fr.FC32: 8, fr.SC16: 4, fr.SC8: 2}[fmt]
    cfg = cfg_of(capi)
    want = ref(x, fmt, scale, cfg)
    rng = np.random.default_rng(7)
    d_in, d_out, d_st = rx.alloc(x.nbytes), rx.alloc(n * 8), rx.alloc(capi.FE_STATE_DTYPE.itemsize)
    try:
        d_in.upload(x)
        d_st.upload(np.zeros(1, capi.FE_STATE_DTYPE))
        pos = 0
        while pos < n:
            k = min(int(rng.integers(1, 9001)), n - pos)
            rx.frontend_dev(cfg, d_st.ptr, d_in.ptr + pos * bps, fmt, k, d_out.ptr + pos * 8, scale)
            pos += k
        same((d_out.download(np.complex64, n), d_st.download(capi.FE_STATE_DTYPE, 1)[0]), want)
    finally:
        d_in.free()
        d_out.free()
        d_st.free()


def test_n_zero_does_nothing(rx):
    from wifirx import capi
    st0 = ref(samples(5000, fr.FC32)[0], fr.FC32, 1.0, cfg_of(capi))[1]
    z, st = run_dev(rx, np.zeros(0, np.complex64), fr.FC32, 1.0, cfg_of(capi), state=st0)
    assert z.size == 0 and st.tobytes() == st0.tobytes()


def test_einval(rx):
    from wifirx import capi
    lib, h = capi.lib(), rx._h
    buf, st = rx.alloc(64 * 1024), rx.alloc(capi.FE_STATE_DTYPE.itemsize + 16)
    st.upload(np.zeros(1, capi.FE_STATE_DTYPE))
    good = cfg_of(capi)
    n = 1000
    src, dst = buf.ptr, buf.ptr + 32 * 1024

    def call(cfg=good, state=st.ptr, i=src, fmt=fr.SC16, scale=1.0, k=n, o=dst):
        return lib.wifirx_frontend(h, C.byref(cfg) if cfg is not None else None, state, i, fmt, scale, k, o)
    try:
        assert call() == capi.OK
        assert lib.wifirx_frontend(None, C.byref(good), st.ptr, src, fr.SC16, 1.0, n, dst) == capi.EINVAL
        for kw in (dict(cfg=None), dict(state=None), dict(i=None), dict(o=None),                            # NULLs
                   dict(fmt=3), dict(fmt=-1),                                                               # unknown fmt
                   dict(cfg=cfg_of(capi, 4)), dict(cfg=cfg_of(capi, 3, 31)), dict(cfg=cfg_of(capi, 3, 12, 7)),
                   dict(cfg=cfg_of(capi, 3, 12, 2, 7)),                                                     # flags, frac_bits, shifts
                   dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),   # integer formats need a scale
                   dict(i=src + 2), dict(fmt=fr.SC8, i=src + 1), dict(fmt=fr.FC32, i=src + 4), dict(o=dst + 4),
                   dict(state=st.ptr + 4),                                                                  # misalignment
                   dict(o=src + 8), dict(o=src), dict(fmt=fr.FC32, i=src, o=src + 8),                       # partial overlap; in == out for integers
                   dict(fmt=fr.FC32, i=dst + 8, o=dst),
                   dict(state=dst + 16), dict(state=src),                                                   # the state inside a buffer
                   dict(k=(1 << 40) + 1)):
            assert call(**kw) == capi.EINVAL, kw
            assert lib.wifirx_last_error(h) != b""
        assert call(fmt=fr.FC32, scale=float("nan")) == capi.OK                 # FC32: scale is not looked at
        assert call(fmt=fr.FC32, i=dst, o=dst) == capi.OK                       # in == out
        assert call(k=0, i=src + 8, o=src) == capi.OK                           # n = 0: nothing overlaps
        assert call(k=0, i=st.ptr + 8, o=st.ptr + 16) == capi.OK                # not the state either: an empty range shares no byte
        rx.sync()
    finally:
        buf.free()
        st.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_rx_impair(rx, n):
    from wifirx import capi
    x, _ = samples(n, fr.FC32, seed=8)
    mu, nu = capi.iq_imbalance(2.0, 10.0)
    dc = 0.3 - 1.7j
    want = fr.rx_impair(x, mu, nu, dc)
    assert np.array_equal(rx.rx_impair(x, mu, nu, dc).view(np.uint32), want.view(np.uint32))               # in place
    d_in, d_out = rx.alloc(n * 8 + 8), rx.alloc(n * 8 + 16)
    try:
        d_in.upload(np.concatenate([np.zeros(1, np.complex64), x]))                                        # both sides 8 bytes off
        rx.rx_impair_dev(d_in.ptr + 8, d_out.ptr + 8, n, mu, nu, dc)
        assert np.array_equal(d_out.download(np.complex64, n + 1)[1:].view(np.uint32), want.view(np.uint32))
    finally:
        d_in.free()
        d_out.free()
    assert np.array_equal(rx.rx_impair(x).view(np.uint32), fr.rx_impair(x).view(np.uint32))                # the identity setting


def test_rx_impair_einval(rx):
    from wifirx import capi
    lib, h = capi.lib(), rx._h
    buf = rx.alloc(4096)
    v = lambda a, b: (C.c_float * 2)(a, b)
    one, zero = v(1, 0), v(0, 0)
    try:
        assert lib.wifirx_rx_impair(h, buf.ptr, buf.ptr, 100, one, zero, zero) == capi.OK
        assert lib.wifirx_rx_impair(h, buf.ptr, buf.ptr + 2048, 100, one, zero, zero) == capi.OK
        assert lib.wifirx_rx_impair(h, buf.ptr, buf.ptr, 0, one, zero, zero) == capi.OK
        for args in ((None, buf.ptr, 100, one, zero, zero), (buf.ptr, None, 100, one, zero, zero), (buf.ptr, buf.ptr, 100, None, zero, zero),
                     (buf.ptr, buf.ptr, 100, one, None, zero), (buf.ptr, buf.ptr, 100, one, zero, None),
                     (buf.ptr + 4, buf.ptr, 100, one, zero, zero), (buf.ptr, buf.ptr + 4, 100, one, zero, zero),
                     (buf.ptr, buf.ptr + 8, 100, one, zero, zero), (buf.ptr + 8, buf.ptr, 100, one, zero, zero),
                     (buf.ptr, buf.ptr, 100, v(float("nan"), 0), zero, zero), (buf.ptr, buf.ptr, 100, one, v(0, float("inf")), zero),
                     (buf.ptr, buf.ptr, 100, one, zero, v(float("-inf"), 0)), (buf.ptr, buf.ptr, (1 << 40) + 1, one, zero, zero)):
            assert lib.wifirx_rx_impair(h, *args) == capi.EINVAL, args
        assert lib.wifirx_rx_impair(None, buf.ptr, buf.ptr, 100, one, zero, zero) == capi.EINVAL
        rx.sync()
    finally:
        buf.free()


def test_host_arrays_in_and_out(rx):
    from wifirx import capi
    x, scale = samples(3 * B + 17, fr.SC16, seed=9)
    cfg = capi.frontend_cfg(dc=True, iq=True)
    z1, st1 = rx.frontend(x[:10000], cfg, scale=scale)
    z2, st2 = rx.frontend(x[10000:], cfg, state=st1, scale=scale)
    same((np.concatenate([z1, z2]), st2), ref(x, fr.SC16, scale, cfg))
    assert [np.atleast_1d(v).view(np.uint32).tolist() for v in capi.frontend_estimate(cfg, st2)] == \
        [np.atleast_1d(v).view(np.uint32).tolist() for v in fr.Frontend(flags=3, state=st2).estimate()]
