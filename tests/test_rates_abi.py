"""The two per-rate entry points are part of the C ABI: declared in include/wifirx.h, exported by libwifirx.so, listed in
capi.EXPORTS; additive (the ABI version and the counter struct are what they were)."""
import ctypes as C
import os
import re

from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wifirx_tx_batch_rates", "wifirx_link_stats_by_rate")


def header():
    with open(os.path.join(ROOT, "include", "wifirx.h")) as f:
        return f.read()


def test_header_declares_both():
    h = header()
    for name in NEW:
        assert re.search(r"^int\s+%s\(wifirx_handle\* h," % name, h, re.M), name
    assert re.search(r"wifirx_tx_batch_rates\(wifirx_handle\* h, const uint8_t\* encoding,", h)
    assert re.search(r"wifirx_link_counts\* total,\s+wifirx_link_counts\* by_rate\);", h)


def test_library_exports_and_capi_lists_both():
    for name in NEW:
        assert name in capi.EXPORTS, name
        assert hasattr(capi.lib(), name), name


def test_abi_version_and_struct_unchanged():
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", header())
    assert capi.ABI_VERSION == 4
    assert capi.lib().wifirx_abi_version() == 4
    assert C.sizeof(capi.LinkCounts) == 72
    assert re.search(r"\}\s*wifirx_link_counts;\s*/\* 72 bytes \*/", header())
