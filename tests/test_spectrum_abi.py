"""The C ABI of the band survey (NUMERICS.md rule 36) as far as it needs no GPU: the six symbols are declared, exported, bound
and listed; the constants; wifirx_spectrum_count and wifirx_spectrum_band equal tests/spectrum_ref.py; every call refuses what
the header says before it looks for a device, with its outputs untouched; and the ABI version, which this feature leaves at 4."""
import ctypes as C
import os
import re

import numpy as np

import spectrum_ref as sr
from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wifirx.h")
SYMBOLS = {"wifirx_spectrum": 14, "wifirx_spectrum_count": 6, "wifirx_spectrum_fold": 9, "wifirx_spectrum_bands": 8,
           "wifirx_spectrum_band": 6, "wifirx_spectrum_table": 4}


def test_symbols_are_declared_exported_bound_and_listed():
    txt = open(HEADER).read()
    for s, n_args in SYMBOLS.items():
        assert re.search(r"\bint\s+%s\(" % s, txt), s + " is not declared in include/wifirx.h"
        assert hasattr(capi.lib(), s), s + " is not exported by libwifirx.so"
        assert getattr(capi.lib(), s).argtypes is not None, s + " is not bound in capi.py"
        assert len(getattr(capi.lib(), s).argtypes) == n_args, s
        assert s in capi.EXPORTS, s + " is not in capi.EXPORTS"


def test_constants():
    txt = open(HEADER).read()

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))

    assert macro("WIFIRX_SPEC_MAX_BANDS") == capi.SPEC_MAX_BANDS == sr.MAX_BANDS == 16
    assert macro("WIFIRX_SPEC_MAX_HOP") == capi.SPEC_MAX_HOP == sr.MAX_HOP == 1 << 20
    assert (macro("WIFIRX_SPEC_RECT"), macro("WIFIRX_SPEC_HANN"), macro("WIFIRX_SPEC_BLACKMAN_HARRIS")) == \
        (capi.SPEC_RECT, capi.SPEC_HANN, capi.SPEC_BLACKMAN_HARRIS) == (sr.RECT, sr.HANN, sr.BLACKMAN_HARRIS) == (0, 1, 2)
    assert (macro("WIFIRX_SPEC_SUM"), macro("WIFIRX_SPEC_MAX")) == (capi.SPEC_SUM, capi.SPEC_MAX) == (sr.SUM, sr.MAX) == (0, 1)
    assert capi.SPEC_N_FFT == sr.N_FFT == (64, 256, 1024, 4096)


def test_abi_version_is_unchanged():
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", open(HEADER).read())


def test_count_equals_the_restatement():
    rng = np.random.default_rng(36)
    for _ in range(400):
        n_fft = int(rng.choice(sr.N_FFT))
        hop = int(rng.integers(1, 3 * n_fft)) if rng.random() < 0.8 else int(rng.integers(1, sr.MAX_HOP + 1))
        avg = int(rng.integers(1, 6)) if rng.random() < 0.8 else int(rng.integers(1, sr.MAX_HOP + 1))
        n_in = int(rng.integers(0, 20 * n_fft)) if rng.random() < 0.7 else int(rng.integers(0, 1 << 40))
        assert capi.spectrum_count(n_fft, hop, avg, n_in) == sr.count(n_fft, hop, avg, n_in), (n_fft, hop, avg, n_in)
    assert capi.spectrum_count(64, 64, 1, 63) == (0, 0) and capi.spectrum_count(64, 64, 1, 64) == (1, 64)
    assert capi.spectrum_count(256, 1, 1 << 20, (1 << 62) - 1) == sr.count(256, 1, 1 << 20, (1 << 62) - 1)


def test_count_refuses_what_the_header_excludes():
    lib = capi.lib()
    r, c = C.c_uint64(7), C.c_uint64(9)
    for n_fft, hop, avg in ((0, 1, 1), (128, 1, 1), (16, 1, 1), (8192, 1, 1), (64, 0, 1), (64, 1, 0), (64, (1 << 20) + 1, 1), (64, 1, (1 << 20) + 1)):
        assert lib.wifirx_spectrum_count(n_fft, hop, avg, 1000, C.byref(r), C.byref(c)) == capi.EINVAL, (n_fft, hop, avg)
    assert lib.wifirx_spectrum_count(64, 1, 1, 1000, None, C.byref(c)) == capi.EINVAL
    assert lib.wifirx_spectrum_count(64, 1, 1, 1000, C.byref(r), None) == capi.EINVAL
    assert lib.wifirx_spectrum_count(64, 1, 1, 1 << 62, C.byref(r), C.byref(c)) == capi.ERANGE
    assert (r.value, c.value) == (7, 9)


def test_band_equals_the_restatement():
    rng = np.random.default_rng(37)
    seen_none = 0
    for _ in range(400):
        n_fft = int(rng.choice(sr.N_FFT))
        fs = float(rng.choice([20e6, 61.44e6, 80e6, 25e6]))
        off, width = float(rng.uniform(-0.6, 0.6) * fs), float(rng.uniform(0.001, 0.5) * fs)
        if rng.random() < 0.3:                                # edges that fall on bin centres
            off, width = float(rng.integers(-n_fft // 2, n_fft // 2)) * fs / n_fft, float(rng.integers(1, n_fft // 2)) * fs / n_fft
        want = sr.band(off, width, fs, n_fft)
        lo, hi = C.c_uint32(7), C.c_uint32(9)
        rc = capi.lib().wifirx_spectrum_band(off, width, fs, n_fft, C.byref(lo), C.byref(hi))
        if want is None:
            seen_none += 1
            assert rc == capi.ERANGE and (lo.value, hi.value) == (7, 9), (off, width, fs, n_fft)
        else:
            assert rc == capi.OK and (lo.value, hi.value) == want == capi.spectrum_band(off, width, fs, n_fft), (off, width, fs, n_fft)
            assert 0 <= want[0] < want[1] <= n_fft
    assert 20 < seen_none < 380
    assert capi.spectrum_band(-25e6, 20e6, 80e6, 256) == (16, 80) and capi.spectrum_band(25e6, 20e6, 80e6, 256) == (176, 240)


def test_band_refuses_what_the_header_excludes():
    lib = capi.lib()
    lo, hi = C.c_uint32(7), C.c_uint32(9)
    nan, inf = float("nan"), float("inf")
    for off, w, fs, n in ((nan, 20e6, 80e6, 256), (inf, 20e6, 80e6, 256), (0.0, nan, 80e6, 256), (0.0, inf, 80e6, 256), (0.0, 0.0, 80e6, 256),
                          (0.0, -1.0, 80e6, 256), (0.0, 20e6, 0.0, 256), (0.0, 20e6, -80e6, 256), (0.0, 20e6, nan, 256), (0.0, 20e6, inf, 256),
                          (0.0, 20e6, 80e6, 128), (0.0, 20e6, 80e6, 0)):
        assert lib.wifirx_spectrum_band(off, w, fs, n, C.byref(lo), C.byref(hi)) == capi.EINVAL, (off, w, fs, n)
    assert lib.wifirx_spectrum_band(0.0, 20e6, 80e6, 256, None, C.byref(hi)) == capi.EINVAL
    assert lib.wifirx_spectrum_band(0.0, 20e6, 80e6, 256, C.byref(lo), None) == capi.EINVAL
    for off, w in ((35e6, 20e6), (-35e6, 20e6), (1e5, 1.0), (0.0, 80e6 + 1e6)):
        assert lib.wifirx_spectrum_band(off, w, 80e6, 256, C.byref(lo), C.byref(hi)) == capi.ERANGE, (off, w)
    assert (lo.value, hi.value) == (7, 9)


def test_table_refuses_a_null_argument():
    lib = capi.lib()
    p, n = C.POINTER(C.c_float)(), C.c_uint32(7)
    for a in ((None, C.byref(p), C.byref(p), C.byref(n)), (C.byref(p), None, C.byref(p), C.byref(n)),
              (C.byref(p), C.byref(p), None, C.byref(n)), (C.byref(p), C.byref(p), C.byref(p), None)):
        assert lib.wifirx_spectrum_table(*a) == capi.EINVAL
    assert n.value == 7 and not p
    hann, bh, tw = capi.spectrum_table()
    assert hann.shape == bh.shape == (4096,) and tw.shape == (4096, 2)


def test_calls_without_a_handle_are_refused():
    lib = capi.lib()
    n = C.c_uint64(7)
    lo, hi = (C.c_uint32 * 16)(0), (C.c_uint32 * 16)(1)
    assert lib.wifirx_spectrum(None, None, 0, 1.0, 0, 64, 64, 1, 0, 0, 1.0, None, 0, C.byref(n)) == capi.EINVAL
    assert lib.wifirx_spectrum_fold(None, None, 0, 64, 1, 0, None, 0, C.byref(n)) == capi.EINVAL
    assert lib.wifirx_spectrum_bands(None, None, 0, 64, 1, lo, hi, None) == capi.EINVAL
    assert n.value == 7
