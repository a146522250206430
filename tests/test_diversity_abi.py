"""wifirx_diversity_combine in the C ABI and the Python surface, on a box without a GPU: the symbol, the signature, the mode
constants.  The call refuses a NULL handle first and a handle needs a device, so every other refused argument is exercised
where a handle exists, in tests/test_gpu_diversity.py."""
import ctypes as C
import inspect
import re

from abi_helpers import _decl, _header, _header_raw, _norm


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    assert re.search(r"\bint\s+wifirx_diversity_combine\s*\(", txt)
    assert "wifirx_diversity_combine" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_diversity_combine")
    assert len(_decl(txt, "wifirx_diversity_combine").split(",")) == 8 == len(capi.lib().wifirx_diversity_combine.argtypes)


def test_argument_list_matches_the_ctypes_signature():
    from wifirx import capi
    assert _norm(_decl(_header(), "wifirx_diversity_combine")) == [
        "wifirx_handle* h", "uint32_t n_ant", "const wifirx_out* in", "uint32_t n_slots", "int mode", "const float* ant_gain",
        "const wifirx_out* out", "uint8_t* used_mask"]
    assert list(capi.lib().wifirx_diversity_combine.argtypes) == [
        C.c_void_p, C.c_uint32, C.POINTER(capi.Out), C.c_uint32, C.c_int, C.POINTER(C.c_float), C.POINTER(capi.Out), C.c_void_p]


def test_mode_constants():
    from wifirx import capi
    raw = _header_raw()
    assert re.search(r"#define\s+WIFIRX_DIV_MRC\s+0\b", raw) and re.search(r"#define\s+WIFIRX_DIV_SELECT\s+1\b", raw)
    assert (capi.DIV_MRC, capi.DIV_SELECT) == (0, 1) and capi.DIV_MODES == {"mrc": 0, "select": 1} and capi.DIV_MAX_ANT == 8


def test_abi_version_and_the_output_struct_stay():
    from wifirx import capi
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", _header_raw())
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert C.sizeof(capi.Out) == 72


def test_a_null_handle_is_refused():
    from wifirx import capi
    out = capi.Out()
    assert capi.lib().wifirx_diversity_combine(None, 2, None, 0, 0, None, C.byref(out), None) == capi.EINVAL
    assert capi.lib().wifirx_diversity_combine(None, 0, None, 0, 7, None, None, None) == capi.EINVAL


def test_python_surface():
    from wifirx import capi
    prm = inspect.signature(capi.WifiRx.diversity_combine_dev).parameters
    assert list(prm) == ["self", "ins", "n_slots", "out", "mode", "ant_gain", "used_mask_ptr"]
    assert (prm["mode"].default, prm["ant_gain"].default, prm["used_mask_ptr"].default) == (capi.DIV_MRC, None, None)
    prm = inspect.signature(capi.WifiRx.demod_diversity).parameters
    assert list(prm)[:6] == ["self", "iqs", "slot_len", "mode", "ant_gain", "soft"]
    assert (prm["mode"].default, prm["ant_gain"].default, prm["soft"].default) == (capi.DIV_MRC, None, False)
