"""wifirx_channelize and wifirx_channelizer_table in the C ABI and the Python surface, on a box without a GPU: the symbols,
the signatures, the table and its refused arguments.  wifirx_channelize refuses a NULL handle first and a handle needs a
device, so every other refused argument of that call is exercised where a handle exists, in tests/test_gpu_channelizer.py."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    for name, n_args in (("wifirx_channelize", 12), ("wifirx_channelizer_table", 3)):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
        assert len(_decl(txt, name).split(",")) == n_args == len(getattr(capi.lib(), name).argtypes), name


def test_argument_lists_match_the_ctypes_signatures():
    from wifirx import capi
    txt = _header()
    assert _norm(_decl(txt, "wifirx_channelize")) == [
        "wifirx_handle* h", "const void* in", "int fmt", "float scale", "const void* hist", "void* hist_out",
        "uint32_t n_channels", "int stacking", "uint64_t n_out", "uint64_t m0", "float* out", "uint64_t out_stride"]
    assert list(capi.lib().wifirx_channelize.argtypes) == [
        C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64,
        C.c_void_p, C.c_uint64]
    assert _norm(_decl(txt, "wifirx_channelizer_table")) == ["uint32_t n_channels", "const float** taps", "uint32_t* n_taps"]
    assert list(capi.lib().wifirx_channelizer_table.argtypes) == [C.c_uint32, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_uint32)]


def test_abi_version_stays():
    from wifirx import capi
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", _header_raw())
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4


def test_table_without_a_device():
    from wifirx import capi
    lib = capi.lib()
    for M in (2, 4, 8):
        p, n = C.POINTER(C.c_float)(), C.c_uint32()
        assert lib.wifirx_channelizer_table(M, C.byref(p), C.byref(n)) == capi.OK and n.value == 24 * M
        h = capi.channelizer_table(M)
        assert h.dtype == np.float32 and h.shape == (24 * M,)
        assert np.array_equal(h, np.ctypeslib.as_array(p, shape=(24 * M,)))
        assert np.isfinite(h).all() and np.array_equal(h, h[::-1])
    p, n = C.POINTER(C.c_float)(), C.c_uint32(7)
    for M in (0, 1, 3, 6, 16):
        assert lib.wifirx_channelizer_table(M, C.byref(p), C.byref(n)) == capi.EINVAL, M
        with pytest.raises(capi.WifiRxError):
            capi.channelizer_table(M)
    assert lib.wifirx_channelizer_table(4, None, C.byref(n)) == capi.EINVAL
    assert lib.wifirx_channelizer_table(4, C.byref(p), None) == capi.EINVAL
    assert n.value == 7


def test_a_null_handle_is_refused():
    from wifirx import capi
    assert capi.lib().wifirx_channelize(None, None, 0, 1.0, None, None, 4, 1, 0, 0, None, 0) == capi.EINVAL


def test_python_surface():
    from wifirx import block, capi
    assert list(inspect.signature(capi.WifiRx.channelize_dev).parameters) == [
        "self", "in_ptr", "fmt", "n_out", "n_channels", "stacking", "out_ptr", "out_stride", "hist_ptr", "hist_out_ptr", "m0",
        "scale"]
    assert capi.CHANNELIZER_CHANNELS == (2, 4, 8) and capi.CHANNELIZER_HIST == 23
    assert [capi.channel_centre(k, 4, 1) for k in range(4)] == [-0.375, -0.125, 0.125, 0.375]
    assert [capi.channel_centre(k, 2, 0) for k in range(2)] == [-0.5, 0.0]
    prm = inspect.signature(block.wifi_phy_rx_wideband.__init__).parameters
    assert list(prm)[:4] == ["self", "n_channels", "stacking", "center_frequency"]
    assert prm["bandwidth"].default == 20e6 and prm["sample_format"].default == "fc32" and prm["sample_scale"].default is None


def test_wideband_block_settles_its_signature_before_it_touches_the_library(monkeypatch):
    from wifirx import block, capi

    class NoDevice:
        def __init__(self, *a, **k):
            raise RuntimeError("no device")
    monkeypatch.setattr(capi, "WifiRx", NoDevice)
    for fmt, sig in (("fc32", [np.complex64]), ("sc16", [(np.int16, 2)]), ("sc8", [(np.int8, 2)])):
        blk = block.wifi_phy_rx_wideband.__new__(block.wifi_phy_rx_wideband)
        with pytest.raises(RuntimeError):
            block.wifi_phy_rx_wideband.__init__(blk, 4, 1, 5.21e9, sample_format=fmt)
        assert blk.in_sig == sig, fmt
        assert blk.frequencies == [5.18e9, 5.20e9, 5.22e9, 5.24e9]
    for bad in (dict(n_channels=3, stacking=1), dict(n_channels=4, stacking=2)):
        with pytest.raises(ValueError):
            block.wifi_phy_rx_wideband(center_frequency=5.21e9, **bad)
    with pytest.raises(ValueError):
        block.wifi_phy_rx_wideband(4, 1, 5.21e9, sample_format="sc12")


def test_fed_blocks_pass_a_failing_handle_on_and_close_half_built(monkeypatch):
    """the three blocks with a front stage and K chains: a handle that cannot be made is the constructor's error, and what
    was built up to there closes without one"""
    from wifirx import block, capi

    class NoDevice:
        def __init__(self, *a, **k):
            raise RuntimeError("no device")
    monkeypatch.setattr(capi, "WifiRx", NoDevice)
    for cls, args in ((block.wifi_phy_rx_wideband, (4, 1, 5.21e9)), (block.wifi_phy_rx_resampled, (25e6,)),
                      (block.wifi_phy_rx_tuned, (80e6,))):
        blk = cls.__new__(cls)
        with pytest.raises(RuntimeError, match="no device"):
            cls.__init__(blk, *args)
        blk.close()
        blk.close()
