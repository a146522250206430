"""wifirx_mac_batch and wifirx_link_stats at the ABI, on a box without a GPU: declared in include/wifirx.h, exported by the
library, bound by capi; additive -- the ABI version stays 4; wifirx_link_counts is 72 bytes for gcc and for ctypes."""
import ctypes
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("wifirx_mac_batch", "wifirx_link_stats")


def test_header_library_and_binding_agree():
    from wifirx import capi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wifirx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(wifirx_[a-z0-9_]+)\s*\(", txt))
    for s in NEW:
        assert s in declared, s
        assert s in capi.EXPORTS, s
        assert hasattr(capi.lib(), s), s
        assert getattr(capi.lib(), s).argtypes is not None, s
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", txt)
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert callable(capi.WifiRx.mac_batch_dev) and callable(capi.WifiRx.mac_batch) and callable(capi.WifiRx.link_stats)


def test_link_counts_layout():
    from wifirx import capi
    import link_ref
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "wifirx.h"\nint main(void){printf("%zu %zu %zu\\n", '
           'sizeof(wifirx_link_counts), offsetof(wifirx_link_counts, frames_psdu_ok), '
           'offsetof(wifirx_link_counts, coded_bit_errors_sq));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert sizes == [72, 32, 64]
    assert ctypes.sizeof(capi.LinkCounts) == 72
    assert tuple(k for k, _ in capi.LinkCounts._fields_) == link_ref.COUNTERS
    assert capi.LinkCounts.frames_psdu_ok.offset == 32 and capi.LinkCounts.coded_bit_errors_sq.offset == 64


def test_link_rates():
    """fer, coded_ber and the standard error of the per-frame BER, from the counters alone"""
    import numpy as np
    from wifirx import capi
    e = np.array([0, 3, 10, 1], np.int64)
    bits = 11 * 288
    c = dict(frames=6, frames_ref=5, frames_good=4, frames_crc_ok=3, frames_psdu_ok=3, frames_crc_ok_wrong=0,
             coded_bits=4 * bits, coded_bit_errors=int(e.sum()), coded_bit_errors_sq=int((e * e).sum()))
    r = capi.link_rates(c)
    per = e / bits
    assert r["fer"] == 1 - 3 / 5
    assert abs(r["coded_ber"] - per.mean()) < 1e-15
    assert abs(r["coded_ber_se"] - per.std() / 2) < 1e-15
    z = capi.link_rates(dict.fromkeys(c, 0))
    assert all(np.isnan(v) for v in z.values())
