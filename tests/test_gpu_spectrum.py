"""wifirx_spectrum, wifirx_spectrum_fold and wifirx_spectrum_bands (wr_spectrum.hip) against tests/spectrum_ref.py, bit for bit:
every n_fft, window, mode and sample format; one row, one full tile of rows, one more than a tile, five; avg 1, 2, 3; hops that
give odd segment starts; the input one sample into its buffer; an input one sample short of a row and exactly a row; infinities,
NaNs and -0 in the first and in a later segment; a stream cut at `consumed`; two calls queued back to back; canaries around every
output; and the refused arguments."""
import ctypes as C

import numpy as np
import pytest

import convert_ref as cr
import spectrum_ref as sr
from bank_helpers import CANARY, alloc_bufs, bits_of, download_fenced, fill, open_rx, same_bits, tile
from wifirx import capi

pytestmark = pytest.mark.gpu

TILE = tile("wr_spectrum.h", "WR_SPEC_TILE")
BPS = {cr.FC32: 8, cr.SC16: 4, cr.SC8: 2}
FORMATS = [cr.FC32, cr.SC16, cr.SC8]
FMT_ID = {cr.FC32: "fc32", cr.SC16: "sc16", cr.SC8: "sc8"}
CASES = [pytest.param(n, fmt, id="%d-%s" % (n, FMT_ID[fmt])) for n in sr.N_FFT for fmt in FORMATS]
WINDOWS = (sr.RECT, sr.HANN, sr.BLACKMAN_HARRIS)
MODES = (sr.SUM, sr.MAX)
N_IN_MAX, ROWS_MAX = 40000, 1 << 15           # samples of an input, floats of a call's rows
FRONT = 24                                    # bytes in front of the rows in the output buffer


@pytest.fixture(scope="module")
def rx():
    yield from open_rx()


@pytest.fixture(scope="module")
def bufs(rx):
    yield from alloc_bufs(rx, inp=(N_IN_MAX + 1) * 8 + 16, out=FRONT + ROWS_MAX * 4 + 64, out2=FRONT + ROWS_MAX * 4 + 64)


def samples(rng, n, fmt):
    """n samples of a format, [n, 2]"""
    if fmt == cr.FC32:
        return rng.standard_normal((n, 2)).astype(np.float32)
    info = np.iinfo(cr.DTYPE[fmt])
    return rng.integers(info.min, info.max + 1, (n, 2)).astype(cr.DTYPE[fmt])


def scale_of(fmt, scale=None):
    if fmt == cr.FC32:
        return float("nan")                                   # not looked at
    return float(cr.SCALE[fmt] if scale is None else np.float32(scale))


def need(n_fft, hop, avg, rows):
    """the fewest samples that give `rows` rows"""
    return (rows * avg - 1) * hop + n_fft if rows else 0


def run_dev(rx, bufs, x, fmt, scale, n_fft, hop, avg, window, mode, norm=1.0, in_off=0, cap_extra=0, out="out"):
    """one call: the rows as float32 [n_rows, n_fft]; checks n_rows against the restatement's count and every byte of the
    output buffer outside the rows"""
    bps, n_in = BPS[fmt], len(x)
    want_rows, _ = sr.count(n_fft, hop, avg, n_in)
    assert n_in <= N_IN_MAX and want_rows * n_fft <= ROWS_MAX
    bufs["inp"].upload(np.concatenate([np.full(in_off * bps, 0x5A, np.uint8), bits_of(x), np.full(16, 0x5A, np.uint8)]))
    fill(bufs[out])
    got = rx.spectrum_dev(bufs["inp"].ptr + in_off * bps, fmt, n_in, n_fft, hop, avg, bufs[out].ptr + FRONT, want_rows + cap_extra,
                          window, mode, norm, scale=scale)
    assert got == want_rows
    raw = download_fenced(bufs[out], [(FRONT, got * n_fft * 4)], "its rows")
    return raw[FRONT:FRONT + got * n_fft * 4].view(np.float32).reshape(got, n_fft)


@pytest.mark.parametrize("n_fft,fmt", CASES)
def test_rows_windows_modes_hops_and_offsets(rx, bufs, n_fft, fmt):
    rng = np.random.default_rng(100 * n_fft + fmt)
    per_tile = max(TILE // n_fft, 1)
    hops, avgs = (n_fft, n_fft // 2, n_fft // 4 + 1, n_fft + 3), (1, 2, 3)
    step, seen = 0, set()
    for rows in sorted({1, per_tile, per_tile + 1, 5}):
        for window in WINDOWS:
            for mode in MODES:
                hop, avg, in_off = hops[step % 4], avgs[step % 3], (step // 4) % 2
                step += 1
                while need(n_fft, hop, avg, rows) + hop - 1 > N_IN_MAX:       # n_fft = 4096: fewer segments, then a shorter hop
                    if avg > 1:
                        avg -= 1
                    else:
                        hop = n_fft // 4 + 1
                seen.add((hop == n_fft + 3 or hop == n_fft // 4 + 1, in_off))
                scale = None if step % 2 else 1.0 / 3.0
                norm = 1.0 if step % 3 else 1.0 / (n_fft * avg)
                x = samples(rng, need(n_fft, hop, avg, rows) + (step % 5) * (hop - 1) // 4, fmt)   # up to hop - 1 samples too many
                got = run_dev(rx, bufs, x, fmt, scale_of(fmt, scale), n_fft, hop, avg, window, mode, norm, in_off, cap_extra=step % 2)
                want = sr.spectrum_format(x, fmt, scale_of(fmt, scale), n_fft, hop, avg, window, mode, norm)
                assert got.shape == (rows, n_fft) and same_bits(got, want), (rows, window, mode, hop, avg, in_off)
    assert seen == {(False, 0), (False, 1), (True, 0), (True, 1)}             # odd segment starts at both buffer offsets


@pytest.mark.parametrize("n_fft,fmt", [(64, cr.SC8), (256, cr.FC32), (1024, cr.SC16), (4096, cr.SC8)], ids=["64-sc8", "256-fc32", "1024-sc16", "4096-sc8"])
def test_one_sample_short_of_a_row_and_exactly_a_row(rx, bufs, n_fft, fmt):
    rng = np.random.default_rng(n_fft)
    hop, avg = n_fft // 2, 2
    n = need(n_fft, hop, avg, 1)
    x = samples(rng, n, fmt)
    assert run_dev(rx, bufs, x[:n - 1], fmt, scale_of(fmt), n_fft, hop, avg, sr.HANN, sr.SUM, cap_extra=3).shape == (0, n_fft)
    assert run_dev(rx, bufs, x[:n_fft - 1], fmt, scale_of(fmt), n_fft, hop, 1, sr.HANN, sr.SUM).shape == (0, n_fft)
    assert run_dev(rx, bufs, x[:0], fmt, scale_of(fmt), n_fft, hop, avg, sr.HANN, sr.SUM).shape == (0, n_fft)
    got = run_dev(rx, bufs, x, fmt, scale_of(fmt), n_fft, hop, avg, sr.HANN, sr.SUM)
    assert got.shape == (1, n_fft) and same_bits(got, sr.spectrum_format(x, fmt, scale_of(fmt), n_fft, hop, avg, sr.HANN, sr.SUM))


@pytest.mark.parametrize("n_fft", [64, 1024, 4096])
@pytest.mark.parametrize("mode", MODES, ids=["sum", "max"])
def test_non_finite_samples_and_negative_zeros(rx, bufs, n_fft, mode):
    """rows of three segments: an infinity in sample 0 of a first segment (every bin inf under a rectangular window: exponent 0
    is not multiplied), an infinity elsewhere, a NaN in a later segment (it sticks under MAX), a row of -0 samples, a row
    with -0 in its last segment.  NaNs stand where the restatement has them; every other value is bit-equal"""
    rng = np.random.default_rng(5 + n_fft)
    hop, avg, rows = n_fft, 3, 6
    if need(n_fft, hop, avg, rows) > N_IN_MAX:
        hop, rows = n_fft // 4, 6
    seg = lambda r, s: (r * avg + s) * hop                    # noqa: E731
    for window in (sr.RECT, sr.BLACKMAN_HARRIS):
        x = samples(rng, need(n_fft, hop, avg, rows), cr.FC32)
        if hop == n_fft:
            x[seg(0, 0), 0] = np.inf
            x[seg(1, 0) + 5, 1] = -np.inf
            x[seg(2, 2) + 7, 0] = np.nan
            x[seg(3, 0):seg(4, 0)] = -0.0
            x[seg(4, 2):seg(5, 0)] = -0.0
        else:                                                 # overlapping segments: one event per stretch of rows
            x[seg(1, 0) + n_fft - 1, 0] = np.inf
            x[seg(4, 1) + n_fft - 1, 1] = np.nan
            x[:seg(0, 2)] = -0.0
        got = run_dev(rx, bufs, x, cr.FC32, scale_of(cr.FC32), n_fft, hop, avg, window, mode)
        want = sr.spectrum(x, n_fft, hop, avg, window, mode)
        nan = np.isnan(want)
        assert nan.any() and not nan.all() and np.isinf(want).any()
        assert np.array_equal(np.isnan(got), nan), window
        assert np.array_equal(bits_of(got[~nan]), bits_of(want[~nan])), window
        if hop == n_fft and window == sr.RECT:
            assert np.isinf(got[0]).all() and np.isinf(want[0]).all()
            assert (got[3] == 0).all() and not np.signbit(got[3]).any()


@pytest.mark.parametrize("n_fft,fmt", [(64, cr.SC8), (256, cr.SC16), (1024, cr.FC32)], ids=["64-sc8", "256-sc16", "1024-fc32"])
def test_a_stream_cut_at_consumed_into_three_calls_is_the_uncut_stream(rx, bufs, n_fft, fmt):
    rng = np.random.default_rng(77 + n_fft)
    hop, avg = n_fft // 4 + 1, 2
    x = samples(rng, need(n_fft, hop, avg, 9) + 11, fmt)
    whole = run_dev(rx, bufs, x, fmt, scale_of(fmt), n_fft, hop, avg, sr.BLACKMAN_HARRIS, sr.SUM, 0.25)
    assert whole.shape[0] == 9 and same_bits(whole, sr.spectrum_format(x, fmt, scale_of(fmt), n_fft, hop, avg, sr.BLACKMAN_HARRIS, sr.SUM, 0.25))
    parts, pos = [], 0
    for end in (need(n_fft, hop, avg, 2) + 3, need(n_fft, hop, avg, 6) + hop - 1, len(x)):
        parts.append(run_dev(rx, bufs, x[pos:end], fmt, scale_of(fmt), n_fft, hop, avg, sr.BLACKMAN_HARRIS, sr.SUM, 0.25, in_off=len(parts) % 2))
        assert capi.spectrum_count(n_fft, hop, avg, end - pos)[0] == parts[-1].shape[0]
        pos += capi.spectrum_count(n_fft, hop, avg, end - pos)[1]
    assert [p.shape[0] for p in parts] == [2, 4, 3]
    assert same_bits(np.concatenate(parts), whole)


def test_two_calls_queued_without_a_sync(rx, bufs):
    """the second call starts at the first call's `consumed` and writes behind its rows; nothing waits between them"""
    n_fft, hop, avg, fmt = 256, 128, 3, cr.SC16
    x = samples(np.random.default_rng(6), need(n_fft, hop, avg, 7), fmt)
    n1 = need(n_fft, hop, avg, 3) + 50
    r1, used = sr.count(n_fft, hop, avg, n1)
    bufs["inp"].upload(bits_of(x))
    fill(bufs["out"])
    a = rx.spectrum_dev(bufs["inp"].ptr, fmt, n1, n_fft, hop, avg, bufs["out"].ptr + FRONT, 7, sr.HANN, sr.MAX)
    b = rx.spectrum_dev(bufs["inp"].ptr + used * 4, fmt, len(x) - used, n_fft, hop, avg, bufs["out"].ptr + FRONT + a * n_fft * 4, 7 - a,
                        sr.HANN, sr.MAX)
    assert (a, b) == (r1, 7 - r1) == (3, 4)
    raw = download_fenced(bufs["out"], [(FRONT, 7 * n_fft * 4)], "the two calls' rows")
    got = raw[FRONT:FRONT + 7 * n_fft * 4].view(np.float32).reshape(7, n_fft)
    assert same_bits(got, sr.spectrum_format(x, fmt, scale_of(fmt), n_fft, hop, avg, sr.HANN, sr.MAX))


@pytest.mark.parametrize("n_fft", [64, 4096])
def test_fold_of_rows(rx, bufs, n_fft):
    rng = np.random.default_rng(8 + n_fft)
    n_rows = 7
    rows = (rng.random((n_rows, n_fft)) * 100).astype(np.float32)
    rows[2] = np.nan
    rows[4, 3], rows[5, n_fft - 1], rows[0, 0] = np.inf, -0.0, np.nan
    bufs["out2"].upload(np.concatenate([np.full(FRONT, 0x5A, np.uint8), bits_of(rows)]))
    for mode in MODES:
        for group in (1, 2, 3, n_rows):
            fill(bufs["out"])
            made = rx.spectrum_fold_dev(bufs["out2"].ptr + FRONT, n_rows, n_fft, group, bufs["out"].ptr + FRONT, n_rows // group, mode)
            assert made == n_rows // group
            raw = download_fenced(bufs["out"], [(FRONT, made * n_fft * 4)], "the folded rows")
            got = raw[FRONT:FRONT + made * n_fft * 4].view(np.float32).reshape(made, n_fft)
            want = sr.fold(rows, group, mode)
            nan = np.isnan(want)
            assert nan.any() and np.array_equal(np.isnan(got), nan) and np.array_equal(bits_of(got[~nan]), bits_of(want[~nan])), (mode, group)
            if group == 1:
                assert same_bits(got, rows)                   # a group of one row is the row, NaN payloads included


@pytest.mark.parametrize("n_fft", sr.N_FFT)
def test_band_powers(rx, bufs, n_fft):
    """widths 1, 63, 64, 65 and N, a band that ends at N, overlapping bands; 1 band and 16"""
    rng = np.random.default_rng(9 + n_fft)
    n_rows = 3
    rows = (rng.random((n_rows, n_fft)) * 100).astype(np.float32)
    rows[1, 5] = np.inf
    bufs["out2"].upload(np.concatenate([np.full(FRONT, 0x5A, np.uint8), bits_of(rows)]))
    N = n_fft
    sixteen = [(0, 1), (7, 70), (0, 64), (1, 65), (3, 68), (0, N), (N - 1, N), (N - 63, N), (N - 65, N), (N // 2 - 32, N // 2 + 32),
               (N // 2 - 33, N // 2 + 32), (5, 6), (0, N), (N - 64, N), (0, 2), (N // 4, 3 * N // 4)]
    sixteen = [(max(lo, 0), min(hi, N)) for lo, hi in sixteen]            # n_fft = 64 has no band of 65 bins
    for edges in ([(0, N)], [(N - 1, N)], [(2, 3)], sixteen):
        fill(bufs["out"])
        rx.spectrum_bands_dev(bufs["out2"].ptr + FRONT, n_rows, n_fft, edges, bufs["out"].ptr + FRONT)
        raw = download_fenced(bufs["out"], [(FRONT, n_rows * len(edges) * 4)], "the band powers")
        got = raw[FRONT:FRONT + n_rows * len(edges) * 4].view(np.float32).reshape(n_rows, len(edges))
        assert same_bits(got, sr.bands(rows, edges)), edges


def test_refused_arguments_leave_every_buffer_alone(rx, bufs):
    lib, h = capi.lib(), rx._h
    nan, inf = float("nan"), float("inf")
    i, o, o2 = bufs["inp"].ptr, bufs["out"].ptr, bufs["out2"].ptr
    n = 1000                                                  # n_fft 64, hop 32, avg 2: 30 segments, 15 rows
    big = 1 << 20
    # (in, fmt, scale, n_in, n_fft, hop, avg, window, mode, norm, rows_out, rows_cap)
    einval = [
        (None, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15), (i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, None, 15),
        (i, 3, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15), (i, -1, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15),
        (i, 1, 0.0, n, 64, 32, 2, 0, 0, 1.0, o, 15), (i, 2, -1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15),
        (i, 1, nan, n, 64, 32, 2, 0, 0, 1.0, o, 15), (i, 2, inf, n, 64, 32, 2, 0, 0, 1.0, o, 15),
        (i, 0, 1.0, n, 64, 32, 2, 3, 0, 1.0, o, 15), (i, 0, 1.0, n, 64, 32, 2, -1, 0, 1.0, o, 15),
        (i, 0, 1.0, n, 64, 32, 2, 0, 2, 1.0, o, 15), (i, 0, 1.0, n, 64, 32, 2, 0, -1, 1.0, o, 15),
        (i, 0, 1.0, n, 0, 32, 2, 0, 0, 1.0, o, 15), (i, 0, 1.0, n, 128, 32, 2, 0, 0, 1.0, o, 15),
        (i, 0, 1.0, n, 16, 32, 2, 0, 0, 1.0, o, 15), (i, 0, 1.0, n, 8192, 32, 2, 0, 0, 1.0, o, 15),
        (i, 0, 1.0, n, 64, 0, 2, 0, 0, 1.0, o, 15), (i, 0, 1.0, n, 64, big + 1, 2, 0, 0, 1.0, o, 15),
        (i, 0, 1.0, n, 64, 32, 0, 0, 0, 1.0, o, 15), (i, 0, 1.0, n, 64, 32, big + 1, 0, 0, 1.0, o, 15),
        (i + 4, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15), (i + 2, 1, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15),
        (i + 1, 2, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15), (i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, o + 2, 15),
        # overlaps: the rows start inside the input, the input starts inside the rows' last float
        (i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, i + n * 8 - 4, 15), (i + 15 * 64 * 4 - 8, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, i, 15),
    ]
    erange = [
        (i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 14), (i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 0),
        (i, 0, 1.0, 1 << 62, 64, 32, 2, 0, 0, 1.0, o, 1 << 62), (i, 2, 1.0, (1 << 64) - 1, 64, 32, 2, 0, 0, 1.0, o, 1 << 62),
        # more than 2^31 - 1 tiles: 2^36 rows of 64 bins
        (i, 0, 1.0, 1 << 42, 64, 64, 1, 0, 0, 1.0, o, 1 << 42),
    ]
    lo, hi = (C.c_uint32 * 17)(*([0] * 17)), (C.c_uint32 * 17)(*([64] * 17))
    bad_lo, bad_hi = (C.c_uint32 * 2)(0, 10), (C.c_uint32 * 2)(64, 10)
    over_hi = (C.c_uint32 * 2)(64, 65)
    fills = {k: fill(d) for k, d in bufs.items()}
    made = C.c_uint64(77)
    for a in einval:
        assert lib.wifirx_spectrum(h, *a, C.byref(made)) == capi.EINVAL, a
    for a in erange:
        assert lib.wifirx_spectrum(h, *a, C.byref(made)) == capi.ERANGE, a
    assert lib.wifirx_spectrum(h, i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, o, 15, None) == capi.EINVAL
    # the fold: (rows, n_rows, n_fft, group, mode, out, out_cap)
    for a in ((None, 6, 64, 2, 0, o, 3), (o2, 6, 64, 2, 0, None, 3), (o2, 6, 128, 2, 0, o, 3), (o2, 6, 64, 0, 0, o, 3), (o2, 6, 64, 2, 2, o, 3),
              (o2 + 2, 6, 64, 2, 0, o, 3), (o2, 6, 64, 2, 0, o + 1, 3), (o2, 6, 64, 2, 0, o2 + 6 * 256 - 4, 3), (o2 + 3 * 256 - 4, 6, 64, 2, 0, o2, 3)):
        assert lib.wifirx_spectrum_fold(h, *a, C.byref(made)) == capi.EINVAL, a
    for a in ((o2, 6, 64, 2, 0, o, 2), (o2, 1 << 40, 64, 2, 0, o, 1 << 40)):
        assert lib.wifirx_spectrum_fold(h, *a, C.byref(made)) == capi.ERANGE, a
    assert lib.wifirx_spectrum_fold(h, o2, 6, 64, 2, 0, o, 3, None) == capi.EINVAL
    # the bands: (rows, n_rows, n_fft, n_bands, lo, hi, out)
    for a in ((None, 3, 64, 2, lo, hi, o), (o2, 3, 64, 2, lo, hi, None), (o2, 3, 64, 2, None, hi, o), (o2, 3, 64, 2, lo, None, o),
              (o2, 3, 64, 0, lo, hi, o), (o2, 3, 64, 17, lo, hi, o), (o2, 3, 100, 2, lo, hi, o), (o2, 3, 64, 2, bad_lo, bad_hi, o),
              (o2, 3, 64, 2, bad_lo, over_hi, o), (o2 + 1, 3, 64, 2, lo, hi, o), (o2, 3, 64, 2, lo, hi, o + 2),
              (o2, 3, 64, 2, lo, hi, o2 + 3 * 256 - 4), (o2 + 3 * 2 * 4 - 4, 3, 64, 2, lo, hi, o2)):
        assert lib.wifirx_spectrum_bands(h, *a) == capi.EINVAL, a
    assert lib.wifirx_spectrum_bands(h, o2, 1 << 31, 64, 2, lo, hi, o) == capi.ERANGE
    assert made.value == 77
    rx.sync()
    for k, d in bufs.items():
        assert np.array_equal(d.download(np.uint8, d.nbytes), fills[k]), k
    assert (bufs["out"].download(np.uint8, 64) == CANARY).all()
    # buffers that only touch are taken: the rows directly behind the input, and fewer than avg segments make no row
    assert lib.wifirx_spectrum(h, i, 0, 1.0, n, 64, 32, 2, 0, 0, 1.0, i + n * 8, 15, C.byref(made)) == capi.OK and made.value == 15
    assert lib.wifirx_spectrum(h, i, 0, 1.0, 64 + 31, 64, 32, 2, 0, 0, 1.0, None, 0, C.byref(made)) == capi.OK and made.value == 0
    assert lib.wifirx_spectrum_fold(h, o2, 6, 64, 7, 0, None, 0, C.byref(made)) == capi.OK and made.value == 0
    assert lib.wifirx_spectrum_bands(h, o2, 0, 64, 2, lo, hi, o) == capi.OK
    rx.sync()
