"""Soft-decision decode_mac on the CPU (NUMERICS.md rule 14): the ABI declares and exports it, and the NumPy reference
(tests/soft_viterbi_ref.py) that the device is checked against is itself pinned -- to the oracle's hard decoder through
+-1 LLRs, to the committed frame error rates of profiles/soft_decode_cpu_fer.json, and on non-finite LLRs."""
import json
import os
import re

import numpy as np
import pytest

import soft_fer_points as sfp
import soft_viterbi_ref as ref
from helpers import make_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_soft_decode():
    txt = open(os.path.join(ROOT, "include", "wifirx.h")).read()
    assert re.search(r"int\s+wifirx_decode_batch_soft\s*\(\s*wifirx_handle\s*\*\s*h\s*,\s*uint32_t\s+n_slots\s*,\s*"
                     r"const\s+wifirx_out\s*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"#define\s+WIFIRX_P_STREAM_SOFT\s+9\b", txt)
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", txt)


def test_library_and_binding_carry_soft_decode():
    from wifirx import capi
    assert hasattr(capi.lib(), "wifirx_decode_batch_soft")
    assert "wifirx_decode_batch_soft" in capi.EXPORTS
    assert capi.P_STREAM_SOFT == 9
    assert callable(capi.WifiRx.decode_batch_soft_dev)


def test_llr_map_is_the_hard_deinterleaver():
    """every transmitted position of a symbol is named exactly once; punctured positions are the 2/3, 3/4 patterns"""
    for enc in range(8):
        m = ref.llr_map(enc)
        kept = m[m >= 0]
        assert sorted(kept.tolist()) == list(range(48 * ref.N_BPSC[enc])), enc
        assert m.size == 2 * ref.N_DBPS[enc]


@pytest.mark.parametrize("enc,snr", [(0, 2.5), (1, 5.0), (2, 6.0), (3, 9.0), (4, 12.0), (5, 15.0), (6, 20.0), (7, 25.0)])
def test_pm1_llrs_reproduce_the_hard_decoder(orc, enc, snr):
    """LLRs of +-1 from the oracle's hard decisions: every metric is a small integer, so the soft reference must return
    oracle.decode_batch's bytes and flags -- pins the reference's maps, trellis, tie rule, descrambler and CRC"""
    iq, slot_len, tx = make_slots(48, enc, psdu_len=60 + 53 * enc, snr_db=snr, seed=40 + enc)
    prm = orc.make_params(max_sym=tx.n_sym, llr_bits=6)
    o = orc.demod_batch(iq, slot_len, prm)
    fr_h = o["frames"].copy()
    hp = orc.decode_batch(fr_h, o["idx"], prm, psdu_stride=1024)
    llr = ref.pm1_llrs(o["frames"], o["idx"], tx.n_sym, 6)
    fr_s, sp = ref.decode_batch(o["frames"], llr, tx.n_sym, psdu_stride=1024)
    assert (fr_h["flags"] & ref.F_DECODED).sum() > 0
    assert np.array_equal(fr_s["flags"], fr_h["flags"])
    assert np.array_equal(sp, hp)


@pytest.fixture(scope="module")
def fer_record():
    with open(os.path.join(ROOT, "profiles", "soft_decode_cpu_fer.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("k", range(len(sfp.POINTS)))
def test_fer_points_match_the_record(orc, fer_record, k):
    """the committed measurement reruns exactly; soft >= hard at every point, and every soft CRC-OK PSDU is the
    transmitted MAC frame"""
    g, snr = sfp.POINTS[k]
    rec = fer_record["points"][k]
    assert (rec["geometry"], rec["snr_db"]) == (g, snr)
    r = sfp.run_point(orc, g, snr, fer_record["frames_per_point"])
    for key in ("hard_crc_ok", "soft_crc_ok", "soft_csi_crc_ok", "hard_delivered", "soft_delivered", "soft_csi_delivered"):
        assert r[key] == rec[key], key
    assert r["soft_crc_ok"] >= r["hard_crc_ok"] and r["soft_csi_crc_ok"] >= r["hard_crc_ok"]
    assert r["soft_delivered"] == r["soft_crc_ok"] and r["soft_csi_delivered"] == r["soft_csi_crc_ok"]


def test_soft_csi_beats_hard_on_config3(fer_record):
    pts = [p for p in fer_record["points"] if p["geometry"] == "config3_sv"]
    assert len(pts) == 3
    for p in pts:
        assert p["soft_csi_delivered"] > 1.5 * p["hard_delivered"] or p["soft_csi_fer"] < p["hard_fer"] - 0.15, p


def test_non_finite_llrs_count_as_zero(orc):
    iq, slot_len, tx = make_slots(24, 3, psdu_len=120, snr_db=12.0, seed=5)
    prm = orc.make_params(max_sym=tx.n_sym, llr_bits=6)
    o = orc.demod_batch(iq, slot_len, prm)
    llr = o["llr"].copy()
    rng = np.random.default_rng(1)
    hit = rng.random(llr.shape) < 0.02
    bad = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=llr.shape)
    llr_bad = np.where(hit, bad, llr).astype(np.float32)
    llr_zero = np.where(hit, np.float32(0), llr).astype(np.float32)
    fa, pa = ref.decode_batch(o["frames"], llr_bad, tx.n_sym, psdu_stride=256)
    fb, pb = ref.decode_batch(o["frames"], llr_zero, tx.n_sym, psdu_stride=256)
    assert (fa["flags"] & ref.F_DECODED).sum() > 0
    assert np.array_equal(fa["flags"], fb["flags"]) and np.array_equal(pa, pb)


def test_frames_without_llr_are_left_alone(orc):
    iq, slot_len, tx = make_slots(16, 4, psdu_len=80, snr_db=20.0, seed=6)
    prm = orc.make_params(max_sym=tx.n_sym, llr_bits=6)
    o = orc.demod_batch(iq, slot_len, prm)
    fr = o["frames"].copy()
    fr["flags"][::2] &= ~np.uint32(ref.F_LLR)
    fs, ps = ref.decode_batch(fr, o["llr"], tx.n_sym, psdu_stride=128)
    assert np.array_equal(fs["flags"][::2], fr["flags"][::2]) and not ps[::2].any()
    assert ((fs["flags"][1::2] & ref.F_CRC_OK) != 0).all()
