"""The C ABI of the receive resampler (NUMERICS.md rule 34) as far as it needs no GPU: the four symbols are declared, exported,
bound and listed; the constants; the prototype the library hands out is the restatement's, bit for bit; the host integers of
wifirx_arb_count / wifirx_arb_hist equal tests/arb_ref.py; capi.arb_ratio; and the ABI version, which this feature leaves at 4."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import arb_ref as ar
from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wifirx.h")
SYMBOLS = ("wifirx_arb_resample", "wifirx_arb_hist", "wifirx_arb_count", "wifirx_arb_table")


def test_symbols_are_declared_exported_bound_and_listed():
    txt = open(HEADER).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, txt), s + " is not declared in include/wifirx.h"
        assert hasattr(capi.lib(), s), s + " is not exported by libwifirx.so"
        assert getattr(capi.lib(), s).argtypes is not None, s + " is not bound in capi.py"
        assert s in capi.EXPORTS, s + " is not in capi.EXPORTS"
    assert len(capi.lib().wifirx_arb_resample.argtypes) == 14


def test_constants():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+WIFIRX_ARB_HIST_MAX\s+(\d+)", txt).group(1)) == capi.ARB_HIST_MAX == ar.HIST_MAX == 128
    assert (capi.ARB_MAX_DEN, capi.ARB_MAX_NUM, capi.ARB_MAX_RATIO) == (ar.MAX_DEN, ar.MAX_NUM, ar.MAX_RATIO) == (512, 2048, 4)
    # HL reaches the constant exactly at the steepest decimation and never passes it
    assert capi.arb_hist(4, 1) == 128 and capi.arb_hist(2048, 512) == 128
    assert max(capi.arb_hist(n, d) for n, d in ar.RATIOS) <= capi.ARB_HIST_MAX


def test_abi_version_is_unchanged():
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", open(HEADER).read())


def test_table_is_the_restatements_bit_for_bit():
    p, n, per = C.POINTER(C.c_float)(), C.c_uint32(), C.c_uint32()
    assert capi.lib().wifirx_arb_table(C.byref(p), C.byref(n), C.byref(per)) == capi.OK
    assert (n.value, per.value) == (4097, 128) == (ar.ENTRIES, ar.PER_UNIT)
    got = capi.arb_table()
    assert got.dtype == np.float32 and got.shape == (4097,)
    assert np.array_equal(got.view(np.uint32), ar.table().view(np.uint32))
    assert capi.lib().wifirx_arb_table(None, C.byref(n), C.byref(per)) == capi.EINVAL
    assert capi.lib().wifirx_arb_table(C.byref(p), None, C.byref(per)) == capi.EINVAL
    assert capi.lib().wifirx_arb_table(C.byref(p), C.byref(n), None) == capi.EINVAL


@pytest.mark.parametrize("num,den", ar.RATIOS)
def test_count_and_hist_equal_the_restatement(num, den):
    assert capi.arb_hist(num, den) == ar.hist_len(num, den)
    rng = np.random.default_rng(num * 1000 + den)
    cases = [(0, E, 0) for E in range(0, 301)]
    big = 1 << 50
    m_big = ar.m_end(num, den, big)
    cases += [(big, int(n), m_big) for n in rng.integers(0, 5000, 40)]
    cases += [(int(j), int(n), int(m)) for j, n, m in zip(rng.integers(0, 1 << 20, 60), rng.integers(0, 4096, 60), rng.integers(0, 1 << 20, 60))]
    for j0, n_in, m0 in cases:
        assert capi.arb_count(num, den, j0, n_in, m0) == ar.count(num, den, j0, n_in, m0), (j0, n_in, m0)


def test_count_and_hist_refuse_what_the_rule_excludes():
    lib = capi.lib()
    n32, n64 = C.c_uint32(7), C.c_uint64(7)
    for num, den in ((0, 1), (1, 0), (5, 1), (1, 5), (4099, 2048), (1027, 513), (2049, 1024), (2049, 512)):
        assert lib.wifirx_arb_hist(num, den, C.byref(n32)) == capi.EINVAL, (num, den)
        assert lib.wifirx_arb_count(num, den, 0, 100, 0, C.byref(n64)) == capi.EINVAL, (num, den)
    assert lib.wifirx_arb_hist(5, 4, None) == capi.EINVAL and lib.wifirx_arb_count(5, 4, 0, 100, 0, None) == capi.EINVAL
    assert (n32.value, n64.value) == (7, 7)
    # the limits themselves are taken, and so is a ratio that only reduces into them
    for num, den in ((2047, 512), (509, 512), (128, 512), (4, 1), (1, 4), (4096, 1024), (40000000, 20000000)):
        assert lib.wifirx_arb_hist(num, den, C.byref(n32)) == capi.OK, (num, den)
        assert n32.value == ar.hist_len(num, den)
    # (j0 + n_in) den and (m0 + n_out) num stay below 2^62
    assert lib.wifirx_arb_count(1, 1, (1 << 62) - 10, 9, 0, C.byref(n64)) == capi.OK
    assert lib.wifirx_arb_count(1, 1, (1 << 62) - 10, 10, 0, C.byref(n64)) == capi.ERANGE
    assert lib.wifirx_arb_count(1, 4, (1 << 60) - 1, 1, 0, C.byref(n64)) == capi.ERANGE
    assert lib.wifirx_arb_count(1, 1, (1 << 64) - 1, 5, 0, C.byref(n64)) == capi.ERANGE
    assert lib.wifirx_arb_count(4, 1, 100, 100, (1 << 60), C.byref(n64)) == capi.ERANGE
    assert lib.wifirx_arb_count(4, 1, 100, 100, (1 << 60) - 1, C.byref(n64)) == capi.OK and n64.value == 0


def test_arb_ratio():
    assert capi.arb_ratio(25e6, 20e6) == (5, 4)
    assert capi.arb_ratio(30.72e6, 20e6) == (192, 125)
    assert capi.arb_ratio(61.44e6, 20e6) == (384, 125)
    assert capi.arb_ratio(20e6, 25e6) == (4, 5)
    assert capi.arb_ratio(61.44e6, 80e6) == (96, 125)
    assert capi.arb_ratio(20e6, 20e6) == (1, 1)
    assert capi.arb_ratio(80e6, 20e6) == (4, 1) and capi.arb_ratio(100e6, 25e6) == (4, 1)
    for a, b in ((100e6, 20e6), (20e6, 100e6), (20e6 + 1, 20e6), (44.1e3, 20e6), (0, 20e6), (20e6, 0), (-1, 20e6)):
        with pytest.raises(ValueError):
            capi.arb_ratio(a, b)


def test_flush_inputs_reach_the_asked_outputs():
    for num, den in ar.RATIOS:
        for n_in in (0, 1, 100, 999):
            for n_out in (0, 1, 57, 1200):
                pad = capi.arb_flush_inputs(num, den, n_in, n_out)
                assert pad == ar.flush_inputs(num, den, n_in, n_out)
                assert ar.count(num, den, 0, n_in + pad, 0) >= n_out
                assert pad == 0 or ar.count(num, den, 0, n_in + pad - 1, 0) < n_out
