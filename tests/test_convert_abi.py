"""The sample-format entry points in the C ABI and the Python surface, on a box without a GPU."""
import inspect
import re

import numpy as np

from abi_helpers import _decl, _header, _header_raw, _norm


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    for name, n_args in (("wifirx_iq_to_f32", 6), ("wifirx_iq_from_f32", 8), ("wifirx_push_iq", 6)):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
        assert len(_decl(txt, name).split(",")) == n_args == len(getattr(capi.lib(), name).argtypes), name


def test_argument_lists():
    txt = _header()
    assert _norm(_decl(txt, "wifirx_iq_to_f32")) == ["wifirx_handle* h", "const void* src", "int fmt", "uint64_t n", "float scale",
                                                     "float* dst"]
    assert _norm(_decl(txt, "wifirx_iq_from_f32")) == ["wifirx_handle* h", "const float* src", "uint64_t n", "float scale", "int fmt",
                                                       "uint32_t bits", "void* dst", "uint64_t* clipped"]
    assert _norm(_decl(txt, "wifirx_push_iq")) == ["wifirx_handle* h", "const void* iq", "size_t n", "int fmt", "float scale",
                                                   "int iq_on_device"]


def test_format_enum():
    from wifirx import capi
    raw = _header_raw()
    for name, value in (("WIFIRX_IQ_FC32", 0), ("WIFIRX_IQ_SC16", 1), ("WIFIRX_IQ_SC8", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), raw), name
    assert (capi.IQ_FC32, capi.IQ_SC16, capi.IQ_SC8) == (0, 1, 2)
    assert capi.IQ_FORMATS == {"fc32": 0, "sc16": 1, "sc8": 2}
    assert capi.IQ_SCALE[capi.IQ_SC16] == 2.0 ** -15 and capi.IQ_SCALE[capi.IQ_SC8] == 2.0 ** -7


def test_additive_beside_an_unchanged_push():
    """the new entry point stands beside wifirx_push, whose signature and ABI version are what they were"""
    from wifirx import capi
    import ctypes as C
    txt = _header()
    assert re.search(r"\bint\s+wifirx_push_iq\s*\(", txt) and hasattr(capi.lib(), "wifirx_push_iq")
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", _header_raw())
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert _norm(_decl(txt, "wifirx_push")) == ["wifirx_handle* h", "const float* iq", "size_t n", "int iq_on_device"]
    assert list(capi.lib().wifirx_push.argtypes) == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert list(inspect.signature(capi.WifiRx.push).parameters) == ["self", "iq"]


def test_python_surface():
    from wifirx import capi
    prm = inspect.signature(capi.WifiRx.push_iq).parameters
    assert list(prm) == ["self", "x", "fmt", "scale"] and prm["fmt"].default is None and prm["scale"].default is None
    for name in ("iq_to_f32", "iq_from_f32", "iq_to_f32_dev", "iq_from_f32_dev", "push_iq_dev"):
        assert callable(getattr(capi.WifiRx, name)), name
    # the format comes from the array: int16 / int8, [n, 2] or flat [2 n]
    for dt, fmt in ((np.int16, capi.IQ_SC16), (np.int8, capi.IQ_SC8)):
        for shape in ((5, 2), (10,)):
            flat, got, n = capi.WifiRx._iq_array(np.zeros(shape, dt))
            assert got == fmt and n == 5 and flat.shape == (10,) and flat.dtype == dt


def test_block_keywords_and_in_sig(monkeypatch):
    from wifirx import block, capi
    prm = inspect.signature(block.wifi_phy_rx.__init__).parameters
    assert prm["sample_format"].default == "fc32" and prm["sample_scale"].default is None

    class NoDevice:                     # the block's signature is settled before it touches the library
        def __init__(self, *a, **k):
            raise RuntimeError("no device")
    monkeypatch.setattr(capi, "WifiRx", NoDevice)
    for fmt, sig in (("fc32", [np.complex64]), ("sc16", [(np.int16, 2)]), ("sc8", [(np.int8, 2)])):
        blk = block.wifi_phy_rx.__new__(block.wifi_phy_rx)
        try:
            block.wifi_phy_rx.__init__(blk, sample_format=fmt)
        except RuntimeError:
            pass
        assert blk.in_sig == sig, fmt
    try:
        block.wifi_phy_rx.__init__(block.wifi_phy_rx.__new__(block.wifi_phy_rx), sample_format="sc12")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown sample_format must be refused")
