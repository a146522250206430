"""The bf16 LLR format on the CPU (NUMERICS.md rule 15): the header and the binding declare WIFIRX_P_LLR_FORMAT and its
values; the NumPy round-to-nearest-even reference the device is checked against (tests/llr_bf16_ref.py) agrees with torch's
CPU bfloat16 conversion on random floats and edge patterns; and a reduced frame-error point of the bf16 soft reference
reruns to the committed record profiles/llr_bf16_cpu_fer.json."""
import json
import os
import re

import numpy as np
import pytest

import llr_bf16_fer_points as bfp
from llr_bf16_ref import bf16_rne, bf16_to_f32, same_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_format():
    txt = open(os.path.join(ROOT, "include", "wifirx.h")).read()
    assert re.search(r"#define\s+WIFIRX_P_LLR_FORMAT\s+10\b", txt)
    assert re.search(r"#define\s+WIFIRX_LLR_F32\s+0\b", txt)
    assert re.search(r"#define\s+WIFIRX_LLR_BF16\s+1\b", txt)
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", txt)


def test_binding_declares_the_format():
    from wifirx import capi
    assert (capi.P_LLR_FORMAT, capi.LLR_F32, capi.LLR_BF16) == (10, 0, 1)
    assert callable(capi.WifiRx.set_llr_format)
    b = np.array([0x3F80, 0xC000, 0x7F80, 0x0001, 0x8000], np.uint16)
    assert capi.bf16_to_f32(b).tolist()[:3] == [1.0, -2.0, float("inf")]
    assert np.array_equal(capi.bf16_to_f32(b).view(np.uint32), b.astype(np.uint32) << 16)


def edge_patterns():
    u = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x00017FFF, 0x00018001,
         0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000,
         0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x00800000, 0x807FFFFF, 0x3F800000, 0xBF7FFFFF]
    return np.array(u, np.uint32).view(np.float32)


def test_rne_agrees_with_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    x = np.concatenate([edge_patterns(),
                        rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        (rng.standard_normal(100000) * 10.0 ** rng.uniform(-40, 38, 100000)).astype(np.float32)])
    t = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert same_bf16(bf16_rne(x), t)
    finite = np.isfinite(x)
    back = bf16_to_f32(bf16_rne(x))
    assert np.array_equal(np.isnan(back), np.isnan(x)) and np.array_equal(back[np.isinf(x)], x[np.isinf(x)])
    # subnormals are kept, not flushed; the largest finite float32 rounds up to inf (ties to even on the boundary)
    assert bf16_rne(np.array([np.uint32(1)], np.uint32).view(np.float32))[0] == 0
    assert bf16_rne(np.array([np.uint32(0x00018000)], np.uint32).view(np.float32))[0] == 0x0002
    assert bf16_rne(np.array([np.uint32(0x7F7FFFFF)], np.uint32).view(np.float32))[0] == 0x7F80
    small = finite & (np.abs(x) < 3.3e38)       # (above, a finite value may round to inf)
    assert (np.abs(back[small] - x[small]) <= np.abs(x[small]) * 2.0 ** -8 + 2.0 ** -133).all()


def test_reduced_point_matches_the_record(orc):
    with open(bfp.OUT) as f:
        rec = json.load(f)
    g, snr, n = bfp.REDUCED
    red = rec["reduced"]
    assert (red["geometry"], red["snr_db"], red["frames"]) == (g, snr, n)
    r = bfp.run_point(orc, g, snr, n)
    for k, v in red.items():
        assert r[k] == v, k
    assert len(rec["points"]) == 4


def test_record_bf16_inside_the_noise():
    """bf16-rounded LLRs deliver within a few frames of float32 at every recorded point"""
    with open(bfp.OUT) as f:
        rec = json.load(f)
    for p in rec["points"]:
        for csi in (0, 1):
            a, b = p["f32_csi%d_delivered" % csi], p["bf16_csi%d_delivered" % csi]
            assert abs(a - b) <= max(3, 3 * np.sqrt(max(a, 1)) / 4), p
