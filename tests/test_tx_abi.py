"""wifirx_tx_batch (the GPU transmitter) in the C ABI: declared by the header, exported by the library, bound by capi."""
import os
import re

from wifirx import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_tx_batch():
    txt = open(os.path.join(ROOT, "include", "wifirx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+wifirx_tx_batch\s*\(", txt)
    assert re.search(r"#define WIFIRX_ABI_VERSION 4\b", txt)         # additive: the version stays


def test_library_exports_tx_batch():
    assert "wifirx_tx_batch" in capi.EXPORTS
    assert hasattr(capi.lib(), "wifirx_tx_batch")


def test_python_surface():
    from wifirx import block
    assert callable(getattr(capi.WifiRx, "tx_batch", None)) and callable(getattr(capi.WifiRx, "tx_batch_dev", None))
    assert callable(getattr(capi.WifiRx, "synth_slots_dev", None))
    assert hasattr(block, "wifi_phy_tx")
