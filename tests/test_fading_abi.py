"""wifirx_channel_fading in the C ABI and the Python surface, on a box without a GPU."""
import inspect
import re

from abi_helpers import _decl, _header


def test_symbol_declared_exported_and_listed():
    from wifirx import capi
    txt = _header()
    assert re.search(r"\bint\s+wifirx_channel_fading\s*\(", txt)
    assert "wifirx_channel_fading" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_channel_fading")


def test_23_arguments_the_last_four_new():
    from wifirx import capi
    decl = _decl(_header(), "wifirx_channel_fading")
    assert len(decl.split(",")) == 23 and len(capi.lib().wifirx_channel_fading.argtypes) == 23
    assert re.search(r"const\s+float\s*\*\s*doppler\s*,\s*float\s+k_factor\s*,\s*uint64_t\s+fade_seed\s*,\s*uint64_t\s+time0\s*$",
                     decl.strip())
    # wifirx_channel_sro's arguments come first, in its order
    norm = lambda s: [re.sub(r"\s+", " ", a).strip() for a in s.split(",")]
    assert norm(decl)[:19] == norm(_decl(_header(), "wifirx_channel_sro"))
    assert list(capi.lib().wifirx_channel_fading.argtypes[:19]) == list(capi.lib().wifirx_channel_sro.argtypes)


def test_additive_version_and_older_signatures_unchanged():
    from wifirx import capi
    txt = _header()
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert len(_decl(txt, "wifirx_channel").split(",")) == 17 and len(capi.lib().wifirx_channel.argtypes) == 17
    assert len(_decl(txt, "wifirx_channel_sro").split(",")) == 19 and len(capi.lib().wifirx_channel_sro.argtypes) == 19


def test_python_keywords():
    from wifirx import block, capi
    for f in (capi.WifiRx.channel, capi.WifiRx.channel_dev):
        prm = inspect.signature(f).parameters
        assert prm["doppler"].default is None and prm["k_factor"].default == 0.0
        assert prm["fade_seed"].default == 0 and prm["time0"].default == 0
    prm = inspect.signature(block.channel_model.__init__).parameters
    assert prm["doppler"].default is None and prm["k_factor"].default == 0.0 and prm["fade_seed"].default == 0
    assert hasattr(block.channel_model, "set_doppler") and hasattr(block.channel_model, "set_k_factor")
    assert capi.DOPPLER_MAX == 2.0 ** -10 and capi.FADE_MAX_TAPS == 16
