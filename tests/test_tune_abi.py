"""The C ABI of the tuner (NUMERICS.md rule 35) as far as it needs no GPU: the two symbols are declared, exported, bound and
listed; the constant; wifirx_tune_inc equals tests/tune_ref.py and refuses what the header says; wifirx_tune refuses its
arguments before it looks for a device; and the ABI version, which this feature leaves at 4."""
import ctypes as C
import os
import re

import numpy as np

import tune_ref as tr
from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wifirx.h")
SYMBOLS = ("wifirx_tune", "wifirx_tune_inc")


def test_symbols_are_declared_exported_bound_and_listed():
    txt = open(HEADER).read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\(" % s, txt), s + " is not declared in include/wifirx.h"
        assert hasattr(capi.lib(), s), s + " is not exported by libwifirx.so"
        assert getattr(capi.lib(), s).argtypes is not None, s + " is not bound in capi.py"
        assert s in capi.EXPORTS, s + " is not in capi.EXPORTS"
    assert len(capi.lib().wifirx_tune.argtypes) == 17 and len(capi.lib().wifirx_tune_inc.argtypes) == 3


def test_constant():
    txt = open(HEADER).read()
    assert int(re.search(r"#define\s+WIFIRX_TUNE_MAX_CHANNELS\s+(\d+)", txt).group(1)) == capi.TUNE_MAX_CHANNELS == tr.MAX_CHANNELS == 8


def test_abi_version_is_unchanged():
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", open(HEADER).read())


def test_tune_inc_equals_the_restatement():
    assert capi.tune_inc(25e6, 80e6) == 0xB000000000000000
    assert capi.tune_inc(-25e6, 80e6) == 0x5000000000000000
    assert capi.tune_inc(0.0, 80e6) == 0
    assert capi.tune_inc(40e6, 80e6) == capi.tune_inc(-40e6, 80e6) == 1 << 63
    rng = np.random.default_rng(35)
    offs = np.concatenate([rng.uniform(-40e6, 40e6, 900), rng.uniform(-400e6, 400e6, 100)])
    for off in offs:
        got = capi.tune_inc(off, 80e6)
        assert got == tr.tune_inc(off, 80e6), off
        assert (got + capi.tune_inc(-off, 80e6)) & tr.M64 == 0, off
    for off, fs in ((1.0, 61.44e6), (-12.5e6, 61.44e6), (5e6, 25e6), (30.72e6, 61.44e6), (1e-3, 80e6), (123456789.0, 7.0)):
        assert capi.tune_inc(off, fs) == tr.tune_inc(off, fs), (off, fs)


def test_tune_inc_refuses_what_the_header_excludes():
    lib = capi.lib()
    v = C.c_uint64(7)
    nan, inf = float("nan"), float("inf")
    for off, fs in ((nan, 80e6), (inf, 80e6), (-inf, 80e6), (1e6, 0.0), (1e6, -80e6), (1e6, nan), (1e6, inf), (1e6, -inf)):
        assert lib.wifirx_tune_inc(off, fs, C.byref(v)) == capi.EINVAL, (off, fs)
    assert lib.wifirx_tune_inc(1e6, 80e6, None) == capi.EINVAL
    assert v.value == 7
    assert lib.wifirx_tune_inc(1e6, 80e6, C.byref(v)) == capi.OK and v.value == tr.tune_inc(1e6, 80e6)


def test_block_refuses_an_offset_that_aliases():
    """checked before any handle is made: 25 MHz in a 61.44 MS/s capture (25 + 10 > 30.72), no offsets, more than eight"""
    import pytest
    from wifirx import block
    with pytest.raises(ValueError, match="alias"):
        block.wifi_phy_rx_tuned(61.44e6, offsets=(25e6,))
    with pytest.raises(ValueError, match="alias"):
        block.wifi_phy_rx_tuned(80e6, offsets=(-25e6, 0.0, 30.5e6))
    with pytest.raises(ValueError):
        block.wifi_phy_rx_tuned(80e6, offsets=())
    with pytest.raises(ValueError):
        block.wifi_phy_rx_tuned(80e6, offsets=(0.0,) * 9)


def test_tune_without_a_handle_is_refused():
    n = C.c_uint64(7)
    inc = (C.c_uint64 * 8)()
    assert capi.lib().wifirx_tune(None, None, 0, 1.0, 0, None, None, 4, 1, 3, inc, None, 0, 0, None, 0, C.byref(n)) == capi.EINVAL
    assert n.value == 7
