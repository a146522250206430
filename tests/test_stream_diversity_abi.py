"""Stream-mode receive diversity in the C ABI and the Python surface, on a box without a GPU: the three symbols and their
signatures, the layout of wifirx_div_stream, the ABI version, the binding's methods, and the block's input ports.  Every call
refuses a NULL handle first and a handle needs a device, so the other refused arguments are exercised where a handle exists, in
tests/test_gpu_stream_diversity.py."""
import ctypes as C
import inspect
import re

import numpy as np

from abi_helpers import _decl, _header, _header_raw, _norm

NAMES = ("wifirx_push_diversity", "wifirx_poll_diversity", "wifirx_detect_multi")


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    for name, n_args in zip(NAMES, (4, 6, 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt)
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
        assert len(_decl(txt, name).split(",")) == n_args == len(getattr(capi.lib(), name).argtypes)


def test_argument_lists_match_the_ctypes_signatures():
    from wifirx import capi
    txt, lib = _header(), capi.lib()
    assert _norm(_decl(txt, "wifirx_push_diversity")) == [
        "wifirx_handle* h", "const wifirx_div_stream* cfg", "const void* const* iq", "size_t n"]
    assert list(lib.wifirx_push_diversity.argtypes) == [C.c_void_p, C.POINTER(capi.DivStream), C.POINTER(C.c_void_p), C.c_size_t]
    assert _norm(_decl(txt, "wifirx_poll_diversity")) == [
        "wifirx_handle* h", "const wifirx_poll_out* out", "uint8_t* used_mask", "wifirx_frame* ant_frames", "uint32_t cap",
        "uint32_t* n_out"]
    assert list(lib.wifirx_poll_diversity.argtypes) == [C.c_void_p, C.POINTER(capi.PollOut), C.c_void_p, C.c_void_p, C.c_uint32,
                                                        C.POINTER(C.c_uint32)]
    assert _norm(_decl(txt, "wifirx_detect_multi")) == [
        "wifirx_handle* h", "uint32_t n_ant", "const float* const* iq_dev", "uint64_t n", "float threshold", "uint64_t* masks_dev",
        "float* A_dev", "float* P_dev"]
    assert list(lib.wifirx_detect_multi.argtypes) == [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_uint64, C.c_float,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]


def test_struct_layout():
    from wifirx import capi
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*wifirx_div_stream\s*;", _header(), flags=re.S).group(1)
    fields = [re.sub(r"\s+", " ", f).strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t n_ant", "int mode", "const float* ant_gain", "int fmt", "float scale", "int iq_on_device"]
    assert [f[0] for f in capi.DivStream._fields_] == ["n_ant", "mode", "ant_gain", "fmt", "scale", "iq_on_device"]
    D = capi.DivStream
    assert (D.n_ant.offset, D.mode.offset, D.ant_gain.offset, D.fmt.offset, D.scale.offset, D.iq_on_device.offset) == (0, 4, 8, 16, 20, 24)
    assert C.sizeof(D) == 32
    assert C.sizeof(capi.PollOut) == 56         # wifirx_poll_out stays as it is: the new outputs are arguments of their own


def test_abi_version_stays_4():
    from wifirx import capi
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", _header_raw())
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4


def test_a_null_handle_is_refused():
    from wifirx import capi
    lib = capi.lib()
    cfg = capi.DivStream(2, 0, None, 0, 1.0, 0)
    n = C.c_uint32(7)
    assert lib.wifirx_push_diversity(None, C.byref(cfg), None, 0) == capi.EINVAL
    assert lib.wifirx_poll_diversity(None, None, None, None, 0, C.byref(n)) == capi.EINVAL
    assert lib.wifirx_detect_multi(None, 1, None, 0, 0.56, None, None, None) == capi.EINVAL


def test_python_surface():
    from wifirx import capi
    W = capi.WifiRx
    prm = inspect.signature(W.push_diversity).parameters
    assert list(prm) == ["self", "iqs", "mode", "ant_gain", "fmt", "scale"]
    assert (prm["mode"].default, prm["ant_gain"].default, prm["fmt"].default, prm["scale"].default) == (capi.DIV_MRC, None, None, None)
    prm = inspect.signature(W.push_diversity_dev).parameters
    assert list(prm)[:5] == ["self", "ptrs", "n", "mode", "ant_gain"] and prm["mode"].default == capi.DIV_MRC
    assert list(inspect.signature(W.flush_diversity).parameters)[:3] == ["self", "mode", "ant_gain"]
    prm = inspect.signature(W.poll_diversity).parameters
    assert list(prm)[:7] == list(inspect.signature(W.poll).parameters)[:7]
    assert list(inspect.signature(W.detect_multi_dev).parameters) == ["self", "iq_ptrs", "n", "threshold", "masks_ptr", "A_ptr", "P_ptr"]


def test_block_signature_and_ports(monkeypatch):
    """wifi_phy_rx(antennas=2) has two input ports of the block's item type under grshim (the handle is stubbed: creating one
    needs a device)"""
    from wifirx import block, capi

    class Stub:
        def __init__(self, **kw):
            self._h = None

        def set_param(self, pid, value):
            pass

    monkeypatch.setattr(capi, "WifiRx", Stub)
    prm = inspect.signature(block.wifi_phy_rx.__init__).parameters
    assert (prm["antennas"].default, prm["diversity"].default, prm["ant_gain"].default) == (1, "mrc", None)
    assert block.wifi_phy_rx().in_sig == [np.complex64]
    b = block.wifi_phy_rx(antennas=2)
    assert b.in_sig == [np.complex64, np.complex64] and b.out_sig is None and b.antennas == 2
    b = block.wifi_phy_rx(antennas=3, sample_format="sc16", diversity="select", ant_gain=[1, 0.5, 2])
    assert b.in_sig == [(np.int16, 2)] * 3 and b.diversity == "select"
    for bad in (dict(antennas=0), dict(antennas=9), dict(antennas=2, diversity="egc"), dict(antennas=2, ant_gain=[1.0]),
                dict(antennas=2, ant_gain=[1.0, -1.0]), dict(antennas=2, ant_gain=[1.0, float("nan")])):
        try:
            block.wifi_phy_rx(**bad)
        except ValueError:
            continue
        raise AssertionError("accepted %r" % (bad,))
