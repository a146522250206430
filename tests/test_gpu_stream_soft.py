"""Stream mode with WIFIRX_P_STREAM_SOFT (wifirx_push / wifirx_poll, soft-decision decode_mac, NUMERICS.md rule 14)
against the references: the oracle's stream driver with llr_bits = 6 for records and LLR rows, tests/soft_viterbi_ref.py
for the decode.  The ten frames of test_gpu_stream.build_stream (all eight rates, mixed lengths) at per-frame SNRs where
soft and hard decisions part; handles created with llr_bits 0, 2 and 6 (the stream's rows reserve 6 bits per carrier
whatever the handle says), WIFIRX_P_LLR_CSI 0 / 1, every chunking and WIFIRX_P_STREAM_BATCH of the hard stream test, and
a stream whose mode changes between flushed parts."""
import functools

import numpy as np
import pytest

import soft_viterbi_ref as ref
from test_gpu_stream import build_stream

pytestmark = pytest.mark.gpu

# per frame of build_stream: low enough that the hard decoder loses frames the soft one keeps, high enough that every
# bits-per-carrier class still has a frame the soft decoder gets right (checked on the references in expected())
SNRS = (4.0, 6.5, 13.0, 24.0, 7.0, 16.0, 10.0, 22.0, 7.0, 6.0)
N_BPSC_OF = np.array(ref.N_BPSC)


@functools.lru_cache(maxsize=None)
def stream():
    x, psdus = build_stream(snr_db=SNRS)
    return x, psdus


@functools.lru_cache(maxsize=None)
def expected(csi):
    """(soft records, soft PSDUs, hard records, hard PSDUs) of the whole stream, from the references alone, and the
    conditions that make the comparison mean something"""
    from oracle import oracle as orc
    x, psdus = stream()
    o = orc.demod_stream(x, orc.make_params(max_sym=511, llr_bits=6, llr_csi=csi), cap=256)
    fr, psdu = ref.decode_batch(o["frames"], o["llr"], 511, psdu_stride=2048)
    prm = orc.make_params(max_sym=511)
    oh = orc.demod_stream(x, prm, cap=256)
    hard_psdu = orc.decode_batch(oh["frames"], oh["idx"], prm, psdu_stride=2048)
    hard = oh["frames"]
    assert len(fr) == len(hard) == len(psdus) and np.array_equal(fr["trigger"], hard["trigger"])
    soft_ok, hard_ok = (fr["flags"] & ref.F_CRC_OK) != 0, (hard["flags"] & ref.F_CRC_OK) != 0
    assert (soft_ok & ~hard_ok).any(), "no frame tells a handle that stayed in hard mode from one in soft mode"
    assert {int(v) for v in N_BPSC_OF[fr["encoding"][soft_ok]]} == {1, 2, 4, 6}
    for k in np.nonzero(soft_ok)[0]:
        assert np.array_equal(psdu[k, :len(psdus[k])], psdus[k])
    return fr, psdu, hard, hard_psdu


def poll_all(rx, got):
    g = rx.poll(cap=64)
    got.append((g["frames"], g["psdu"]))


def assert_frames(frames, psdu, want_fr, want_psdu):
    assert np.array_equal(frames, want_fr), (frames, want_fr)
    for k in range(len(frames)):
        if frames["flags"][k] & ref.F_DECODED:
            L = int(frames["psdu_len"][k])
            assert np.array_equal(psdu[k, :L], want_psdu[k, :L]), k


@pytest.mark.parametrize("chunk,batch", [(777, 0), (4096, 0), (100000, 0), (10**7, 0), (777, 20000), (4096, 1 << 20)])
@pytest.mark.parametrize("csi", [0, 1])
@pytest.mark.parametrize("llr_bits", [0, 2, 6])
def test_soft_stream_matches_the_references(llr_bits, csi, chunk, batch):
    from wifirx import capi
    x, _ = stream()
    fr, want_psdu, _, _ = expected(csi)
    rx = capi.WifiRx(max_sym=511, llr_bits=llr_bits)
    try:
        rx.set_param(capi.P_STREAM_SOFT, 1)
        rx.set_param(capi.P_LLR_CSI, csi)
        rx.set_param(capi.P_STREAM_BATCH, batch)
        got = []
        for p in range(0, x.size, chunk):
            rx.push(x[p:p + chunk])
            poll_all(rx, got)
        rx.flush()
        poll_all(rx, got)
    finally:
        rx.close()
    frames = np.concatenate([g[0] for g in got])
    psdu = np.concatenate([g[1] for g in got])
    # the records of a soft-mode stream are those of a handle with llr_bits = 6 (WIFIRX_F_LLR set: the rows exist, though
    # wifirx_poll has no LLR output), whatever cfg.llr_bits is -- include/wifirx.h at WIFIRX_P_STREAM_SOFT
    assert ((fr["flags"] & ref.F_LLR) != 0).all()
    assert_frames(frames, psdu, fr, want_psdu)


@pytest.mark.parametrize("csi", [0, 1])
def test_mode_switch_between_flushed_parts(csi):
    """soft, then hard, then soft again, the stream flushed (in a gap between frames) before each change: every part equals
    its own reference -- "batches run after the call use it" """
    from wifirx import capi
    from wifirx import txgen
    x, _ = stream()
    fr, soft_psdu, hard, hard_psdu = expected(csi)
    specs = [(0, 60), (2, 294), (4, 500), (7, 1000)]          # the first four frames of build_stream: where part one ends
    cut1 = sum(100 + txgen.frame_samples(l, e) + 1000 for e, l in specs) - 500
    assert fr["trigger"][3] < cut1 < fr["trigger"][4]
    cut2 = int(fr["trigger"][7]) - 600                         # inside the gap in front of frame 7
    assert int(fr["trigger"][6]) + txgen.frame_samples(294, 3) + 200 < cut2          # frame 6 (QPSK 3/4, 294 B) has ended
    parts = [(1, x[:cut1]), (0, x[cut1:cut2]), (1, x[cut2:])]
    rx = capi.WifiRx(max_sym=511, llr_bits=0)
    got = []
    try:
        rx.set_param(capi.P_LLR_CSI, csi)
        for soft, seg in parts:
            rx.set_param(capi.P_STREAM_SOFT, soft)
            for p in range(0, seg.size, 4096):
                rx.push(seg[p:p + 4096])
                poll_all(rx, got)
            rx.flush()
            poll_all(rx, got)
    finally:
        rx.close()
    frames = np.concatenate([g[0] for g in got])
    psdu = np.concatenate([g[1] for g in got])
    want_fr = np.concatenate([fr[:4], hard[4:7], fr[7:]])
    want_psdu = np.concatenate([soft_psdu[:4], hard_psdu[4:7], soft_psdu[7:]])
    assert ((want_fr["flags"][4:7] & ref.F_LLR) == 0).all() and not np.array_equal(fr[4:7], hard[4:7])
    assert_frames(frames, psdu, want_fr, want_psdu)
