"""wifirx_decode_batch_soft and the stream's soft mode on the MI355X (NUMERICS.md rule 14) against the NumPy reference
(tests/soft_viterbi_ref.py) fed with the oracle's LLRs: PSDUs and flags bit for bit at every rate, mixed rates and
lengths, batches below and above one wave's 64 frames, frames at max_sym, frames without WIFIRX_F_LLR, llr_csi 0 / 1,
AWGN and SV taps; +-1 LLRs reproduce wifirx_decode_batch; the CPU-recorded gain holds on the device; the block with
soft_decision=True delivers what the reference decodes from the oracle's stream."""
import json
import os

import numpy as np
import pytest

import soft_fer_points as sfp
import soft_viterbi_ref as ref
from wifirx import txgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (40, 150, 300)
MAX_SYM = txgen.n_sym_for(300, 0)          # the longest frame (BPSK 1/2, 300 B) sits at max_sym


@pytest.fixture(scope="module")
def capi():
    from wifirx import capi
    return capi


def mixed_slots(n, snr_db, taps, seed):
    """n slots, frame k of rate k % 8 and length LENS[(k // 8) % 3] (all 8 rates, mixed lengths in one batch)"""
    rng = np.random.default_rng(seed)
    encs = np.arange(n) % 8
    lens = np.array(LENS)[(np.arange(n) // 8) % 3]
    sig = [txgen.encode_psdus(txgen.make_psdus(1, int(ln), seed=seed * 1000 + k), int(e)).samples[0]
           for k, (e, ln) in enumerate(zip(encs, lens))]
    n_max = max(s.size for s in sig)
    frames = np.zeros((n, n_max), np.complex64)
    for k, s in enumerate(sig):
        frames[k, :s.size] = s
    slot_len = ((160 + n_max + 320 + 63) // 64) * 64
    t = None
    if taps is not None:
        t = taps[np.arange(n) % taps.shape[0]]
    x = txgen.impair(frames, snr_db, cfo=rng.uniform(-sfp.CFO_20PPM, sfp.CFO_20PPM, n), lead=160, total=slot_len,
                     seed=seed + 17, taps=t)
    return x.reshape(-1), slot_len


def gpu_soft(capi, iq, slot_len, n, max_sym, llr_bits, csi, psdu_stride=512):
    rx = capi.WifiRx(max_sym=max_sym, llr_bits=llr_bits, device=0)
    try:
        rx.set_param(capi.P_LLR_CSI, csi)
        dev = rx.alloc_out(n, psdu_stride=psdu_stride)
        d_iq = rx.alloc(iq.nbytes).upload(iq)
        try:
            rx.demod_batch_dev(d_iq.ptr, slot_len, n, dev)
            rx.decode_batch_soft_dev(n, dev)
            rx.sync()
            return rx.download_out(dev, n)
        finally:
            d_iq.free()
            rx.free_out(dev)
    finally:
        rx.close()


@pytest.mark.parametrize("n,snr,sv,llr_bits,csi", [
    (40, 12.0, False, 6, 0), (200, 12.0, False, 6, 1), (200, 22.0, True, 6, 1), (136, 22.0, True, 6, 0),
    (200, 14.0, False, 2, 1),          # llr_bits 2: the 16- and 64-QAM frames carry no LLRs and stay as they are
])
def test_soft_decode_equals_reference(capi, orc, n, snr, sv, llr_bits, csi):
    taps = np.load(os.path.join(ROOT, "tests", "golden", "sv_taps.npy")) if sv else None
    iq, slot_len = mixed_slots(n, snr, taps, seed=n + int(snr) + 7 * csi + llr_bits)
    r = gpu_soft(capi, iq, slot_len, n, MAX_SYM, llr_bits, csi)
    o = orc.demod_batch(iq, slot_len, orc.make_params(max_sym=MAX_SYM, llr_bits=llr_bits, llr_csi=csi), n_threads=8)
    assert np.array_equal(r["llr"], o["llr"]), "LLRs differ from the oracle"
    fr, psdu = ref.decode_batch(o["frames"], o["llr"], MAX_SYM, psdu_stride=512)
    assert np.array_equal(r["frames"], fr)
    assert np.array_equal(r["psdu"], psdu)
    dec = (fr["flags"] & ref.F_DECODED) != 0
    assert dec.sum() > n // 3 and ((fr["flags"] & ref.F_CRC_OK) != 0).sum() > 0
    assert (fr["n_sym"][dec] == MAX_SYM).any()
    if llr_bits == 2:
        no_llr = ((o["frames"]["flags"] & ref.F_COMPLETE) != 0) & ((o["frames"]["flags"] & ref.F_LLR) == 0)
        assert no_llr.sum() > 0 and np.array_equal(r["frames"][no_llr], o["frames"][no_llr])


def test_pm1_llrs_give_the_hard_decoder(capi):
    """+-1 LLRs built from the device's decisions: wifirx_decode_batch_soft == wifirx_decode_batch, bytes and flags"""
    n = 200
    iq, slot_len = mixed_slots(n, 10.0, None, seed=99)
    rx = capi.WifiRx(max_sym=MAX_SYM, llr_bits=6, device=0)
    try:
        dev = rx.alloc_out(n, psdu_stride=512, want_hbits=True)
        d_iq = rx.alloc(iq.nbytes).upload(iq)
        rx.demod_batch_dev(d_iq.ptr, slot_len, n, dev)
        rx.sync()
        r0 = rx.download_out(dev, n)
        dev["llr"].upload(ref.pm1_llrs(r0["frames"], r0["idx"], MAX_SYM, 6))
        rx.decode_batch_soft_dev(n, dev)
        rx.sync()
        rs = rx.download_out(dev, n)
        dev["frames"].upload(r0["frames"])
        dev["psdu"].upload(np.zeros(n * 512, np.uint8))
        rx.decode_batch_dev(n, dev)
        rx.sync()
        rh = rx.download_out(dev, n)
        d_iq.free()
        rx.free_out(dev)
    finally:
        rx.close()
    assert ((rh["frames"]["flags"] & ref.F_DECODED) != 0).sum() > n // 2
    assert np.array_equal(rs["frames"], rh["frames"]) and np.array_equal(rs["psdu"], rh["psdu"])


@pytest.mark.parametrize("k", range(len(sfp.POINTS)))
def test_fer_points_on_the_device(capi, k):
    """the CPU record's CRC-OK counts, plain and channel-state-weighted, from the device's LLRs and soft decoder"""
    with open(os.path.join(ROOT, "profiles", "soft_decode_cpu_fer.json")) as f:
        rec = json.load(f)
    g, snr = sfp.POINTS[k]
    p = rec["points"][k]
    x, slot_len, max_sym, tx = sfp.point_frames(g, snr, rec["frames_per_point"])
    n = tx.shape[0]
    for csi, tag in ((0, "soft"), (1, "soft_csi")):
        r = gpu_soft(capi, x, slot_len, n, max_sym, 6, csi, psdu_stride=320)
        assert int(((r["frames"]["flags"] & ref.F_CRC_OK) != 0).sum()) == p[tag + "_crc_ok"], tag
        assert int(sfp.delivered(r["frames"], r["psdu"], tx).sum()) == p[tag + "_delivered"], tag


def test_argument_checks(capi):
    import ctypes as C
    rx = capi.WifiRx(max_sym=8, llr_bits=6, device=0)
    rx0 = capi.WifiRx(max_sym=8, llr_bits=0, device=0)
    try:
        dev = rx.alloc_out(4, psdu_stride=64)
        out = rx._out_struct(dev)
        lib = capi.lib()
        assert lib.wifirx_decode_batch_soft(rx._h, 0, C.byref(out)) == capi.OK
        out_nollr = rx._out_struct(dict(dev, llr=None))
        assert lib.wifirx_decode_batch_soft(rx._h, 4, C.byref(out_nollr)) == capi.EINVAL
        assert lib.wifirx_decode_batch_soft(rx0._h, 4, C.byref(out)) == capi.EINVAL
        host = capi.Out(out.frames, None, out.llr, None, out.psdu, 64, 0, None, None, None)
        assert lib.wifirx_decode_batch_soft(rx._h, 4, C.byref(host)) == capi.EINVAL
        assert lib.wifirx_set_param(rx._h, capi.P_STREAM_SOFT, 2.0) == capi.EINVAL
        assert lib.wifirx_set_param(rx._h, capi.P_STREAM_SOFT, 1.0) == capi.OK
        assert lib.wifirx_set_param(rx._h, capi.P_STREAM_SOFT, 0.0) == capi.OK
        rx.free_out(dev)
    finally:
        rx.close()
        rx0.close()


def run_block(x, soft):
    from wifirx import block, grshim
    got = []
    blk = block.wifi_phy_rx(bandwidth=20e6, publish_carrier=False, soft_decision=soft)
    assert blk.get_soft_decision() == soft
    grshim.msg_connect(blk, "mac_out", grshim.sink_block(got.append), "in")
    grshim.run_stream(blk, x, chunk=8192)
    blk.close()
    return [grshim.to_python(m) if not isinstance(m, tuple) else m for m in got]


def test_block_soft_decision_delivers_the_reference_pdus(orc):
    """a padded low-SNR recording (QPSK 1/2, AWGN near the hard decoder's FER of 0.5): the block with soft_decision=True
    publishes exactly the PDUs the reference decodes from the oracle's stream (llr_bits 6, llr_csi 1), and no fewer than
    the hard block"""
    x, slot_len, _, tx = sfp.point_frames("qpsk12_awgn", 6.5, 48)
    x = np.concatenate([x, np.zeros(2000, np.complex64)])
    o = orc.demod_stream(x, orc.make_params(max_sym=511, llr_bits=6, llr_csi=1), cap=512)
    fr, psdu = ref.decode_batch(o["frames"], o["llr"], 511, psdu_stride=2048)
    want = [psdu[i, :fr["psdu_len"][i] - 4] for i in range(len(fr)) if fr["flags"][i] & ref.F_CRC_OK]
    soft = run_block(x, True)
    hard = run_block(x, False)
    assert len(soft) == len(want) and len(soft) >= len(hard) and len(soft) > 0
    for (meta, blob), w in zip(soft, want):
        assert np.array_equal(np.asarray(blob, np.uint8), w)
