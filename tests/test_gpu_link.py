"""wifirx_mac_batch and wifirx_link_stats (wr_link.hip) through the C ABI, every comparison exact:
  * mac_batch_dev == link_ref.mac_batch for host, device and Philox payloads: every length of the list, mixed lengths in one
    call, row strides 294 / 304 / 1528, 1 .. 4097 frames, rows at every byte alignment; a 0xA5-filled buffer keeps its fill
    behind every PSDU and in front of the first; argument errors are refused on the host and leave the buffer as it was;
  * link_stats == link_ref.link_stats on uploaded hand-made batches of every class, with and without hbits, the per-frame
    arrays, the PSDUs, the decisions;
  * config 3's full sweep (26 points x 4096 frames, hard and soft decode_mac): the device counters and frame_err == what
    NumPy computes from the downloaded buffers;
  * block.mac -> wifi_phy_tx -> channel_model -> wifi_phy_rx: the payloads come back in order."""
import math
import os
import time

import numpy as np
import pytest

import link_ref
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTHS = (0, 1, 3, 262, 266, 1500)
FILL = 0xA5
PAD = 64
ADDR = (bytes([0x10, 0x22, 0x33, 0x44, 0x55, 0x66]), bytes(range(1, 7)), bytes([0xAA, 0xBB, 0xCC, 0xDD, 0xEE, 0x0F]))   # dst, src, bss


@pytest.fixture(scope="module")
def rx():
    r = capi.WifiRx(max_sym=7, device=0)
    yield r
    r.close()


def run_mac(rx, n, stride, kind, lens, shift=0, **kw):
    """mac_batch_dev into a FILL-ed buffer, PAD + shift bytes in; returns (whole buffer, expected whole buffer)"""
    lens = np.broadcast_to(np.asarray(lens, np.uint32), (n,))
    width = int(lens.max(initial=0))
    rng = np.random.default_rng(n * 1000 + stride + width)
    total = PAD + shift + n * stride + PAD
    buf = rx.alloc(total).upload(np.full(total, FILL, np.uint8))
    d_pay = None
    pay = None
    try:
        if kind == "philox":
            rx.mac_batch_dev(buf.ptr + PAD + shift, stride, n, None, payload_len=lens, **kw)
        else:
            pay = rng.integers(0, 256, (n, max(width, 1) + 3), dtype=np.uint8)        # rows wider than the payloads
            if kind == "host":
                rx.mac_batch_dev(buf.ptr + PAD + shift, stride, n, pay, payload_len=lens, **kw)
            else:
                d_pay = rx.alloc(pay.nbytes + 1).upload(np.concatenate([[0], pay.reshape(-1)]).astype(np.uint8))
                rx.mac_batch_dev(buf.ptr + PAD + shift, stride, n, d_pay.ptr + 1, payload_len=lens, payload_stride=pay.shape[1], **kw)
        got = buf.download(np.uint8, total)
    finally:
        buf.free()
        if d_pay is not None:
            d_pay.free()
    want = np.full(total, FILL, np.uint8)
    ref = link_ref.mac_batch(n, pay, payload_len=lens, seq0=kw.get("seq0", 0), addr=kw.get("addr"),
                             payload_seed=kw.get("payload_seed", 0))
    want[PAD + shift:PAD + shift + n * stride] = link_ref.mac_rows(ref, stride, FILL).reshape(-1)
    return got, want


@pytest.mark.parametrize("kind", ["host", "device", "philox"])
def test_mac_batch_every_length(rx, kind):
    for length in LENGTHS:
        for stride in (28 + length, 1528):
            got, want = run_mac(rx, 65, stride, kind, length, seq0=0xFF0, payload_seed=0x1234567800000009)
            assert np.array_equal(got, want), (length, stride)


@pytest.mark.parametrize("kind", ["host", "device", "philox"])
@pytest.mark.parametrize("stride", [294, 304, 1528])
def test_mac_batch_mixed_lengths_strides_and_counts(rx, kind, stride):
    mixed = (0, 1, 3, 262, 266) if stride < 1528 else LENGTHS
    for n in (1, 63, 64, 65, 4097):
        lens = np.array([mixed[(k * 7 + n) % len(mixed)] for k in range(n)], np.uint32)
        got, want = run_mac(rx, n, stride, kind, lens, seq0=4090, payload_seed=77)
        assert np.array_equal(got, want), n


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_mac_batch_rows_at_every_byte_alignment(rx, shift):
    for kind in ("host", "philox"):
        for stride in (293, 295):
            lens = np.array([(0, 1, 3, 262, 265)[k % 5] for k in range(130)], np.uint32)
            got, want = run_mac(rx, 130, stride, kind, lens, shift=shift, addr=ADDR, seq0=1, payload_seed=1 << 40)
            assert np.array_equal(got, want), (kind, stride)


def test_mac_batch_host_convenience_and_tx(rx):
    """mac_batch (host rows) and the hand-over on the device: wifirx_tx_batch(psdu_on_device) directly behind it"""
    p = rx.mac_batch(33, None, payload_len=266, seq0=5, payload_seed=3)
    ref = link_ref.mac_batch(33, None, payload_len=266, seq0=5, payload_seed=3)
    assert p.shape == (33, 294) and np.array_equal(p, np.stack(ref))
    pays = [bytes([k]) * (k % 9) for k in range(20)]
    q = rx.mac_batch(20, pays)
    assert np.array_equal(q, link_ref.mac_rows(link_ref.mac_batch(20, pays), 28 + 8, 0))
    n, enc = 33, 7
    flen = txgen.frame_samples(294, enc)
    d_psdu, rows = rx.alloc(n * 294), rx.alloc(n * flen * 8)
    try:
        rx.mac_batch_dev(d_psdu.ptr, 294, n, None, payload_len=266, seq0=5, payload_seed=3)
        rx.tx_batch_dev(rows.ptr, n * flen, d_psdu.ptr, enc, psdu_len=np.full(n, 294, np.uint32), psdu_stride=294, row_len=flen)
        got = rows.download(np.complex64, n * flen).reshape(n, flen)
    finally:
        d_psdu.free()
        rows.free()
    assert np.array_equal(got, rx.tx_batch(p, enc))


def test_mac_batch_argument_errors(rx):
    n, stride = 8, 304
    buf = rx.alloc(n * stride).upload(np.full(n * stride, FILL, np.uint8))
    pay = np.zeros((n, 266), np.uint8)
    bad = [
        (capi.EINVAL, lambda: rx.mac_batch_dev(None, stride, n, None, payload_len=266)),
        (capi.EINVAL, lambda: rx.mac_batch_dev(buf.ptr, 1600, n, None, payload_len=1501)),
        (capi.EINVAL, lambda: rx.mac_batch_dev(buf.ptr, 1600, n, None, payload_len=[0] * 7 + [1501])),
        (capi.EINVAL, lambda: rx.mac_batch_dev(buf.ptr, stride, n, pay, payload_len=[266] * 7 + [267])),
        (capi.ERANGE, lambda: rx.mac_batch_dev(buf.ptr, 293, n, None, payload_len=266)),
        (capi.ERANGE, lambda: rx.mac_batch_dev(buf.ptr, 290, n, pay, payload_len=[0] * 7 + [263])),
    ]
    try:
        for code, fn in bad:
            with pytest.raises(capi.WifiRxError) as e:
                fn()
            assert e.value.code == code, e.value
        rx.mac_batch_dev(buf.ptr, stride, 0, None, payload_len=266)            # nothing to do: fine
        rx.sync()
        assert (buf.download(np.uint8, n * stride) == FILL).all()
    finally:
        buf.free()


# ---- link_stats ----

def upload_side(rx, side, psdu=True, idx=True, hbits=True):
    d = dict(frames=rx.alloc(side["frames"].nbytes).upload(side["frames"]), psdu_stride=0)
    if psdu:
        d["psdu"], d["psdu_stride"] = rx.alloc(side["psdu"].nbytes).upload(side["psdu"]), side["psdu"].shape[1]
    if idx:
        d["idx"] = rx.alloc(side["idx"].nbytes).upload(side["idx"])
    if hbits:
        d["hbits"] = rx.alloc(side["hbits"].nbytes).upload(side["hbits"])
    return d


def check_stats(rx, n, d_rx, d_ref, h_rx, h_ref, per_frame):
    r = rx.link_stats(n, d_rx, d_ref, per_frame=per_frame)
    counts, err, cls = link_ref.link_stats(h_rx, h_ref, rx.max_sym)
    assert {k: r[k] for k in link_ref.COUNTERS} == counts
    assert r["fer"] == 1.0 - counts["frames_psdu_ok"] / counts["frames_ref"]
    if per_frame:
        try:
            assert np.array_equal(r["frame_err"].download(np.uint32, n), err)
            assert np.array_equal(r["frame_class"].download(np.uint8, n), cls)
        finally:
            r["frame_err"].free()
            r["frame_class"].free()
    return counts


def test_link_stats_hand_made(rx):
    rng = np.random.default_rng(2026)
    n, max_sym = 10_000, rx.max_sym
    classes = rng.integers(0, 8, n)
    h_rx, h_ref = link_ref.hand_made_batch(rng, classes, rng.integers(0, 8, n), rng.choice([1, max_sym], n), max_sym,
                                           rx_stride=64, ref_stride=59)
    sub = lambda side, *keys: {k: (v if k in keys or k == "frames" else None) for k, v in side.items()}
    d_rx, d_ref = upload_side(rx, h_rx), upload_side(rx, h_ref)
    pick = lambda d, *keys: {k: v for k, v in d.items() if k in keys or k in ("frames", "psdu_stride")}
    try:
        seen = []
        for per_frame in (False, True):
            # hbits on both sides; idx alone; hbits on one side only (-> idx)
            seen.append(check_stats(rx, n, d_rx, d_ref, h_rx, h_ref, per_frame))
            seen.append(check_stats(rx, n, pick(d_rx, "psdu", "idx"), pick(d_ref, "psdu", "idx"),
                                    sub(h_rx, "psdu", "idx"), sub(h_ref, "psdu", "idx"), per_frame))
            seen.append(check_stats(rx, n, d_rx, pick(d_ref, "psdu", "idx"), h_rx, sub(h_ref, "psdu", "idx"), per_frame))
            # ref->psdu absent; ref->idx (and hbits) absent
            c = check_stats(rx, n, d_rx, pick(d_ref, "idx", "hbits"), h_rx, sub(h_ref, "idx", "hbits"), per_frame)
            assert c["frames_crc_ok"] == c["frames_psdu_ok"] == c["frames_crc_ok_wrong"] == 0 and c["coded_bits"] > 0
            c = check_stats(rx, n, d_rx, pick(d_ref, "psdu"), h_rx, sub(h_ref, "psdu"), per_frame)
            assert c["coded_bits"] == c["coded_bit_errors"] == 0 and c["frames_psdu_ok"] > 0
        assert all(s == seen[0] for s in seen)
        assert seen[0]["frames_good"] == int((classes >= 4).sum()) and seen[0]["frames_psdu_ok"] == int((classes == 5).sum())
        assert seen[0]["frames_crc_ok_wrong"] == int(((classes == 3) | (classes == 4)).sum())
        # small batches: fewer frames than one workgroup's waves, and none
        for m in (1, 3, 5):
            r = rx.link_stats(m, d_rx, d_ref)
            cut = lambda side: {k: v[:m] for k, v in side.items()}
            assert {k: r[k] for k in link_ref.COUNTERS} == link_ref.link_stats(cut(h_rx), cut(h_ref), max_sym)[0]
        assert rx.link_stats(0, d_rx, d_ref)["frames"] == 0
    finally:
        for d in (d_rx, d_ref):
            rx.free_out(d)


def test_link_stats_argument_errors(rx):
    import ctypes as C
    n = 4
    fr = rx.alloc(n * 32).upload(np.zeros(n * 32, np.uint8))
    dec = rx.alloc(n * rx.max_sym * 48 + 16).upload(np.zeros(n * rx.max_sym * 48 + 16, np.uint8))
    cnt = capi.LinkCounts()
    out = lambda frames, on_dev=1, idx=None: capi.Out(frames, idx, None, None, None, 0, on_dev, None, None, None)
    call = lambda a, b, c: capi.lib().wifirx_link_stats(rx._h, n, a, b, None, None, c)
    good = out(fr.ptr)
    try:
        assert call(None, C.byref(good), C.byref(cnt)) == capi.EINVAL
        assert call(C.byref(good), None, C.byref(cnt)) == capi.EINVAL
        assert call(C.byref(good), C.byref(good), None) == capi.EINVAL
        assert call(C.byref(out(None)), C.byref(good), C.byref(cnt)) == capi.EINVAL
        assert call(C.byref(good), C.byref(out(None)), C.byref(cnt)) == capi.EINVAL
        assert call(C.byref(out(fr.ptr, 0)), C.byref(good), C.byref(cnt)) == capi.EINVAL          # host buffers
        assert call(C.byref(good), C.byref(out(fr.ptr, 0)), C.byref(cnt)) == capi.EINVAL
        mis = out(fr.ptr, 1, dec.ptr + 4)
        assert call(C.byref(mis), C.byref(mis), C.byref(cnt)) == capi.EINVAL                      # idx not 16-byte aligned
        assert call(C.byref(good), C.byref(good), C.byref(cnt)) == capi.OK and cnt.frames == n and cnt.frames_ref == 0
    finally:
        fr.free()
        dec.free()


# ---- config 3, the full sweep ----

SLOT, LEAD, ENC, PSDU_LEN = 1472, 160, 7, 294
CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def test_config3_sweep_device_counters_equal_host_bookkeeping():
    """tools/loopback_per.py's set-up, 5 .. 30 dB in steps of 1 dB, 4096 frames per point, hard and soft decode_mac.
    (Measured on an MI355X: see profiles/README.md for the time this test took.)"""
    t_start = time.perf_counter()
    n, seed = 4096, 1
    n_sym, nb = txgen.n_sym_for(PSDU_LEN, ENC), txgen.RATE_TABLE[ENC][0]
    taps = np.load(os.path.join(GOLD, "sv_taps.npy")).astype(np.complex64)
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, chan_est=capi.EQ_LS, device=0)
    d_psdu, rows, iq = rx.alloc(n * PSDU_LEN), rx.alloc(n * SLOT * 8), rx.alloc(n * SLOT * 8)
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=PSDU_LEN - 28, payload_seed=seed)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                    lead=LEAD, row_len=SLOT)
    ref = rx.alloc_out(n, want_hbits=True)
    ref["psdu"], ref["psdu_stride"] = d_psdu, PSDU_LEN
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    try:
        rx.demod_batch_dev(rows.ptr, SLOT, n, ref)                     # the transmitted decisions: the clean rows
        rx.sync()
        h_ref = rx.download_out(ref, n)
        assert ((h_ref["frames"]["flags"] & capi.F_COMPLETE) != 0).all()
        assert np.array_equal(h_ref["psdu"], np.stack(link_ref.mac_batch(n, None, payload_len=PSDU_LEN - 28, payload_seed=seed)))
        idx_tx = h_ref["idx"].reshape(n, -1)
        total = {k: 0 for k in link_ref.COUNTERS}
        first = {}
        for snr in range(5, 31):
            cfo = np.random.default_rng(1000 * snr + seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
            rx.channel_dev(rows.ptr, iq.ptr, n * SLOT, n, row_len=SLOT, taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)),
                           noise_voltage=1.0, seed=9000 + snr + (seed << 32))
            rx.demod_batch_dev(iq.ptr, SLOT, n, dev)
            for soft in (False, True):
                (rx.decode_batch_soft_dev if soft else rx.decode_batch_dev)(n, dev)
                r = rx.link_stats(n, dev, ref, per_frame=True)
                try:
                    h = rx.download_out(dev, n)
                    counts, err, cls = link_ref.link_stats(h, h_ref, n_sym)
                    assert {k: r[k] for k in link_ref.COUNTERS} == counts, (snr, soft)
                    d_err = r["frame_err"].download(np.uint32, n)
                    assert np.array_equal(d_err, err) and np.array_equal(r["frame_class"].download(np.uint8, n), cls)
                    good = (cls & 1) != 0
                    per_frame = POPCOUNT[h["idx"].reshape(n, -1)[good] ^ idx_tx[good]].sum(axis=1, dtype=np.int64)
                    assert np.array_equal(d_err[good], per_frame) and (d_err[~good] == 0xFFFFFFFF).all()
                    assert abs(r["coded_ber"] - per_frame.mean() / (n_sym * 48 * nb)) < 1e-12
                finally:
                    r["frame_err"].free()
                    r["frame_class"].free()
                assert counts["frames_crc_ok_wrong"] == 0, (snr, soft)
                if not soft:
                    first.setdefault(snr, counts)
                for k in total:
                    total[k] += counts[k]
        # so that the sweep cannot pass empty (profiles/loopback_per_config3.json: FER 0.44 at 30 dB, 58 % good at 5 dB)
        assert total["frames_psdu_ok"] > 0 and total["coded_bit_errors"] > 0
        assert first[5]["frames_good"] < first[5]["frames"] == n
        assert first[30]["frames_psdu_ok"] > first[5]["frames_psdu_ok"]
    finally:
        rx.free_out(dev)
        rx.free_out(ref)                                               # frees d_psdu with it
        rows.free()
        iq.free()
        rx.close()
    print("config 3 sweep: 26 points x %d frames, hard + soft: %.1f s" % (n, time.perf_counter() - t_start))


# ---- through the blocks ----

def test_loop_back_through_the_blocks_with_the_mac_block():
    """block.mac -> wifi_phy_tx -> x gain (25 dB) -> channel_model -> wifi_phy_rx, the set-up of test_gpu_channel's loop-back
    where every frame arrives: the mac_out PDUs, sliced [24:], are the payloads handed to `app in`, in order"""
    from wifirx import block, grshim
    rng = np.random.default_rng(2025)
    n_frames, enc = 200, 2
    payloads = [rng.integers(0, 256, int(rng.integers(1, 372)), dtype=np.uint8).tobytes() for _ in range(n_frames)]
    mac = block.mac()
    tx = block.wifi_phy_tx(encoding=enc, pad_front=100, pad_tail=1000)
    grshim.msg_connect(mac, grshim.intern("phy out"), tx, grshim.intern("mac_in"))
    for p in payloads:
        mac._handlers[grshim.intern("app in")](grshim.make_pdu({}, np.frombuffer(p, np.uint8)))
    parts = []
    while True:
        buf = np.empty(50000, np.complex64)
        k = tx.work([], [buf])
        if k == 0:
            break
        parts.append(buf[:k].copy())
    tx.close()
    x = np.concatenate(parts) * np.float32(math.sqrt(10 ** (25 / 10)))
    ch = block.channel_model(noise_voltage=1, frequency_offset=10e-6 * 5.89e9 / 10e6, epsilon=1.0, taps=[1.0], noise_seed=0)
    y = np.empty_like(x)
    for pos in range(0, x.size, 60000):
        k = min(60000, x.size - pos)
        assert ch.work([x[pos:pos + k]], [y[pos:pos + k]]) == k
    ch.close()
    rxb = block.wifi_phy_rx(bandwidth=20e6, frequency=5.89e9, publish_carrier=False)
    got = []
    grshim.msg_connect(rxb, "mac_out", grshim.sink_block(got.append), "in")
    for pos in range(0, y.size, 30000):
        k = min(30000, y.size - pos)
        assert rxb.work([y[pos:pos + k]], []) == k
    rxb.stop()
    rxb.close()
    assert len(got) == n_frames, len(got)
    for k, (meta, vec) in enumerate(got):
        assert bytes(np.asarray(vec, np.uint8))[24:] == payloads[k], k
