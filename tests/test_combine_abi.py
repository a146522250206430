"""wifirx_combine in the C ABI and the Python surface, on a box without a GPU: the symbol, the signature and the block's
arguments.  wifirx_combine refuses a NULL handle first and a handle needs a device, so every other refused argument is
exercised where a handle exists, in tests/test_gpu_combine.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    assert re.search(r"\bint\s+wifirx_combine\s*\(", txt)
    assert "wifirx_combine" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_combine")
    assert len(_decl(txt, "wifirx_combine").split(",")) == 11 == len(capi.lib().wifirx_combine.argtypes)


def test_argument_list_matches_the_ctypes_signature():
    from wifirx import capi
    assert _norm(_decl(_header(), "wifirx_combine")) == [
        "wifirx_handle* h", "const float* in", "uint64_t in_stride", "const float* gains", "const float* hist", "float* hist_out",
        "uint32_t n_channels", "int stacking", "uint64_t n_in", "uint64_t m0", "float* out"]
    assert list(capi.lib().wifirx_combine.argtypes) == [
        C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint64,
        C.c_uint64, C.c_void_p]


def test_abi_version_stays():
    from wifirx import capi
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", _header_raw())
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4


def test_a_null_handle_is_refused():
    from wifirx import capi
    assert capi.lib().wifirx_combine(None, None, 0, None, None, None, 4, 1, 0, 0, None) == capi.EINVAL


def test_python_surface():
    from wifirx import block, capi, grshim
    assert list(inspect.signature(capi.WifiRx.combine_dev).parameters) == [
        "self", "in_ptr", "in_stride", "n_in", "n_channels", "stacking", "out_ptr", "gains", "hist_ptr", "hist_out_ptr", "m0"]
    assert list(inspect.signature(capi.WifiRx.combine).parameters) == ["self", "streams", "stacking", "gains"]
    prm = inspect.signature(block.wideband_combiner.__init__).parameters
    assert list(prm) == ["self", "n_channels", "stacking", "gains", "device"]
    assert (prm["n_channels"].default, prm["stacking"].default, prm["gains"].default, prm["device"].default) == (4, 1, None, 0)
    assert issubclass(block.wideband_combiner, grshim.sync_interpolator) and issubclass(grshim.sync_interpolator, grshim.sync_block)
    assert hasattr(block.wideband_combiner, "set_gains") and hasattr(block.wideband_combiner, "close")


def test_block_settles_its_signature_before_it_touches_the_library(monkeypatch):
    from wifirx import block, capi

    class NoDevice:
        def __init__(self, *a, **k):
            raise RuntimeError("no device")
    monkeypatch.setattr(capi, "WifiRx", NoDevice)
    for M in (2, 4, 8):
        blk = block.wideband_combiner.__new__(block.wideband_combiner)
        with pytest.raises(RuntimeError):
            block.wideband_combiner.__init__(blk, M, 0, gains=[0.5] * M)
        assert blk.in_sig == [np.complex64] * M and blk.out_sig == [np.complex64] and blk.interpolation() == M
        assert np.array_equal(blk.gains, np.full(M, 0.5, np.float32))
    # refused before the library is touched: ValueError, not NoDevice's RuntimeError
    for bad in (dict(n_channels=3, stacking=1), dict(n_channels=4, stacking=2), dict(n_channels=4, gains=[1.0] * 3),
                dict(n_channels=2, gains=[1.0, float("inf")])):
        with pytest.raises(ValueError):
            block.wideband_combiner(**bad)
