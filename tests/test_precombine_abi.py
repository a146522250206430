"""wifirx_precombine in the C ABI and the Python surface, on a box without a GPU: the symbol, the signature, the constants.
The call refuses a NULL handle first and a handle needs a device, so every other refused argument is exercised where a
handle exists, in tests/test_gpu_precombine.py."""
import ctypes as C
import inspect
import re

from abi_helpers import _decl, _header, _header_raw, _norm


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    assert re.search(r"\bint\s+wifirx_precombine\s*\(", txt)
    assert "wifirx_precombine" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_precombine")
    assert len(_decl(txt, "wifirx_precombine").split(",")) == 9 == len(capi.lib().wifirx_precombine.argtypes)


def test_argument_list_matches_the_ctypes_signature():
    from wifirx import capi
    assert _norm(_decl(_header(), "wifirx_precombine")) == [
        "wifirx_handle* h", "uint32_t n_ant", "const float* const* iq_dev", "uint32_t slot_len", "uint32_t n_slots", "uint32_t iters",
        "float* out_dev", "float* weights_dev", "void* stats_dev"]
    assert list(capi.lib().wifirx_precombine.argtypes) == [
        C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]


def test_constants_and_the_stats_row():
    from wifirx import capi
    assert re.search(r"#define\s+WIFIRX_PRE_DEGENERATE\s+1u?\b", _header_raw())
    assert (capi.PRE_DEGENERATE, capi.PRE_MAX_ANT, capi.PRE_MAX_ITERS) == (1, 8, 4)
    assert capi.PRE_STATS_DTYPE.itemsize == 16 and capi.PRE_STATS_DTYPE.names == ("lambda", "trace", "ref", "flags")
    import precombine_ref as pr
    assert pr.STATS_DTYPE == capi.PRE_STATS_DTYPE and (pr.MAX_ANT, pr.MAX_ITERS, pr.DEGENERATE) == (8, 4, 1)


def test_abi_version_stays():
    from wifirx import capi
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", _header_raw())
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4


def test_a_null_handle_is_refused():
    from wifirx import capi
    ptrs = (C.c_void_p * 2)(4096, 8192)
    assert capi.lib().wifirx_precombine(None, 2, ptrs, 64, 0, 2, 16384, None, None) == capi.EINVAL
    assert capi.lib().wifirx_precombine(None, 0, None, 0, 0, 9, None, None, None) == capi.EINVAL


def test_python_surface():
    from wifirx import capi
    prm = inspect.signature(capi.WifiRx.precombine_dev).parameters
    assert list(prm) == ["self", "iq_ptrs", "slot_len", "n_slots", "out_ptr", "iters", "weights_ptr", "stats_ptr"]
    assert (prm["iters"].default, prm["weights_ptr"].default, prm["stats_ptr"].default) == (2, None, None)
    prm = inspect.signature(capi.WifiRx.precombine).parameters
    assert list(prm) == ["self", "iqs", "slot_len", "iters"] and prm["iters"].default == 2
    prm = inspect.signature(capi.WifiRx.demod_precombined).parameters
    assert list(prm) == ["self", "iqs", "slot_len", "iters", "soft", "psdu_stride"]
    assert (prm["iters"].default, prm["soft"].default, prm["psdu_stride"].default) == (2, False, 2048)
