"""wifirx_tx_batch, the GPU transmitter (wr_tx.hip), through the C ABI and the blocks:
  * bit for bit NUMERICS.md rule 16 (tests/tx_ref.py) and within 1e-6 of txgen, all 8 encodings, host and device PSDUs;
  * every sample of every row written (NaN-filled buffers), row_off = packet_pad2's stream, deterministic;
  * argument errors refused on the host, before any launch;
  * noiseless loop-back through demod + decode_mac, and one million distinct frames through the device channel;
  * config 5 (six images) through wifi_phy_tx -> wifi_phy_rx."""
import ctypes as C
import os

import numpy as np
import pytest

import tx_ref
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

LENGTHS = (1, 24, 100, 294, 1500, 4095)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN_WORD = np.uint32(0x7FC0DEAD)


@pytest.fixture(scope="module")
def rx():
    r = capi.WifiRx(max_sym=64, llr_bits=0, device=0)
    yield r
    r.close()


def rand_psdus(n, length, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, length), dtype=np.uint8)


def nan_buf(rx, n_samples):
    buf = rx.alloc(n_samples * 8)
    buf.upload(np.full(n_samples * 2, NAN_WORD, dtype=np.uint32))
    return buf


def ref_frames(psdus, enc, seeds):
    return [tx_ref.encode(np.frombuffer(bytes(p), np.uint8)[None], enc, [int(s)])[0] for p, s in zip(psdus, seeds)]


@pytest.mark.parametrize("enc", range(8))
def test_bit_exact_host_psdus_mixed_lengths(rx, enc):
    """one call per encoding with every length mixed, host PSDUs (stride = the longest), mixed seeds"""
    rng = np.random.default_rng(enc)
    psdus = [rand_psdus(1, L, 10 * enc + k)[0].tobytes() for k, L in enumerate(LENGTHS * 2)]
    seeds = rng.integers(1, 128, size=len(psdus))
    lead = 37
    rows = rx.tx_batch(psdus, enc, seeds=seeds, lead=lead)
    for i, (p, s) in enumerate(zip(psdus, seeds)):
        want = tx_ref.encode(np.frombuffer(p, np.uint8)[None], enc, [int(s)])[0]
        f = want.size
        assert np.array_equal(rows[i, lead:lead + f], want), (enc, len(p))
        assert np.abs(rows[i, lead:lead + f] - txgen.encode_psdus(np.frombuffer(p, np.uint8)[None], enc, [int(s)]).samples[0]).max() <= 1e-6
        assert not rows[i, :lead].any() and not rows[i, lead + f:].any()


@pytest.mark.parametrize("enc", range(8))
def test_bit_exact_device_psdus_wide_stride(rx, enc):
    """device PSDUs with a stride beyond the longest PSDU, the default seeds (i % 127) + 1, equal lengths per call"""
    for L in LENGTHS:
        n = 4 if L > 1000 else 16
        p = rand_psdus(n, L, 1000 + 10 * enc + L)
        stride = L + 45
        host = np.zeros((n, stride), np.uint8)
        host[:, :L] = p
        host[:, L:] = 0xA5                                   # bytes behind a PSDU must not be read as data
        d_psdu = rx.alloc(host.nbytes).upload(host)
        f = txgen.frame_samples(L, enc)
        row = f + 3
        out = nan_buf(rx, n * row)
        rx.tx_batch_dev(out.ptr, n * row, d_psdu.ptr, enc, psdu_len=np.full(n, L, np.uint32), psdu_stride=stride,
                        row_len=row)
        got = out.download(np.complex64, n * row).reshape(n, row)
        d_psdu.free(); out.free()
        want = tx_ref.encode(p, enc)
        assert np.array_equal(got[:, :f], want), (enc, L)
        assert np.abs(got[:, :f] - txgen.encode_psdus(p, enc).samples).max() <= 1e-6
        assert not got[:, f:].any()


def test_fixed_rows_every_sample_written(rx):
    """NaN-filled buffer, odd row length, a buffer start that is 8 but not 16 bytes aligned: zeros outside every frame"""
    n, L, enc, lead = 50, 77, 5, 9
    p = rand_psdus(n, L, 3)
    f = txgen.frame_samples(L, enc)
    row = lead + f + 17                                         # odd
    out = nan_buf(rx, n * row + 3)
    rx.tx_batch_dev(out.ptr + 8, n * row, p, enc, lead=lead, row_len=row)
    got = out.download(np.complex64, n * row + 3)
    assert np.isnan(got[0]) and np.isnan(got[n * row + 1:]).all(), "samples outside the rows were touched"
    rows = got[1:1 + n * row].reshape(n, row)
    assert not np.isnan(rows).any()
    assert np.array_equal(rows[:, lead:lead + f], tx_ref.encode(p, enc))
    assert not rows[:, :lead].any() and not rows[:, lead + f:].any()
    out.free()


def test_row_off_is_packet_pad_stream(rx):
    enc = 0
    lens = [40, 294, 41, 1500, 1, 100, 2000, 333]
    psdus = [rand_psdus(1, L, 50 + L)[0].tobytes() for L in lens]
    seeds = (np.arange(len(psdus)) % 127) + 1
    frames = ref_frames(psdus, enc, seeds)
    rows = [100 + fr.size + 1000 for fr in frames]
    row_off = np.concatenate([[5], 5 + np.cumsum(rows)]).astype(np.uint64)   # the rows start 5 samples into the buffer
    total = int(row_off[-1])
    out = nan_buf(rx, total + 2)
    rx.tx_batch_dev(out.ptr, total, psdus, enc, lead=100, row_off=row_off)
    a = out.download(np.complex64, total + 2)
    want = np.concatenate([txgen.packet_pad(fr[None], 100, 1000) for fr in frames])
    assert np.isnan(a[:5]).all() and np.isnan(a[total:]).all()
    assert np.array_equal(a[5:total], want)
    rx.tx_batch_dev(out.ptr, total, psdus, enc, lead=100, row_off=row_off)
    b = out.download(np.complex64, total + 2)
    assert a[5:total].tobytes() == b[5:total].tobytes()
    s = rx.tx_batch(psdus, enc, lead=100, row_off=row_off - np.uint64(5))
    assert s.tobytes() == a[5:total].tobytes()             # the host form of the same call
    out.free()


def test_argument_errors_launch_nothing(rx):
    lib = capi.lib()
    p = rand_psdus(4, 100, 1)
    lens = np.full(4, 100, np.uint32)
    f = txgen.frame_samples(100, 2)
    n_s = 4 * (f + 10) + 64
    out = nan_buf(rx, n_s)
    canary = out.download(np.uint8, n_s * 8)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(enc=2, psdu=p, stride=100, ln=lens, seeds=None, n=4, samples=-1, cap=n_s, row_off=None, row_len=f + 10, lead=0):
        return lib.wifirx_tx_batch(rx._h, enc, P(psdu), 0, stride, P(ln), P(seeds), n,
                                   out.ptr if samples == -1 else samples, cap, P(row_off), row_len, lead)

    bad_len = lens.copy(); bad_len[2] = 0
    big_len = lens.copy(); big_len[1] = 4096
    cases = [
        (capi.EINVAL, dict(enc=8)), (capi.EINVAL, dict(enc=-1)), (capi.EINVAL, dict(ln=bad_len)),
        (capi.EINVAL, dict(ln=big_len)), (capi.EINVAL, dict(seeds=np.array([1, 2, 0, 3], np.uint8))),
        (capi.EINVAL, dict(seeds=np.array([1, 128, 5, 3], np.uint8))), (capi.EINVAL, dict(samples=None)),
        (capi.EINVAL, dict(row_off=np.array([0, f, 2 * f, 2 * f - 1, 4 * f], np.uint64))),
        (capi.EINVAL, dict(stride=99)),
        (capi.ERANGE, dict(row_len=f - 1)), (capi.ERANGE, dict(lead=11)), (capi.ERANGE, dict(cap=4 * (f + 10) - 1)),
        (capi.ERANGE, dict(row_off=np.array([0, f, 2 * f, 3 * f, 4 * f - 1], np.uint64))),
        (capi.ERANGE, dict(row_off=np.array([0, f, 2 * f, 3 * f, n_s + 1], np.uint64), row_len=0)),
    ]
    for code, kw in cases:
        assert call(**kw) == code, kw
    assert call(n=0) == capi.OK
    rx.sync()
    assert out.download(np.uint8, n_s * 8).tobytes() == canary.tobytes(), "a refused call wrote samples"
    assert call() == capi.OK
    rx.sync()
    got = out.download(np.complex64, n_s)[:4 * (f + 10)].reshape(4, f + 10)
    assert np.array_equal(got[:, :f], tx_ref.encode(p, 2))
    out.free()


@pytest.mark.parametrize("enc", range(8))
def test_noiseless_loopback(enc):
    """GPU TX into fixed slots, then demod + decode_mac: every PSDU back, CRC ok, decisions = the transmitted indices"""
    max_sym = 64
    lens = [L for L in (28, 60, 100, 294, 700, 1500) if txgen.n_sym_for(L, enc) <= max_sym]
    rx = capi.WifiRx(max_sym=max_sym, llr_bits=0, device=0)
    try:
        for L in lens:
            n = 24
            p = txgen.make_psdus(n, L, seed=enc * 100 + L)
            f = txgen.frame_samples(L, enc)
            slot = 160 + f + 240
            slot += slot % 2
            rows = rx.tx_batch(p, enc, lead=160, row_len=slot)
            r = rx.demod_batch(rows.reshape(-1), slot, decode=True, psdu_stride=((L + 15) // 16) * 16)
            tx = txgen.encode_psdus(p, enc)
            ok = (r["frames"]["flags"] & capi.F_CRC_OK) != 0
            assert ok.all(), (enc, L, int(ok.sum()))
            assert np.array_equal(r["psdu"][:, :L], p)
            assert np.array_equal(r["idx"][:, :tx.n_sym], tx.data_idx)
    finally:
        rx.close()


N_BIG, SLOT, LEAD, ENC, PSDU_LEN, SUBSET = 1_000_000, 4608, 160, 2, 294, 4096


def _vector_psdus(n, length, seed):
    """txgen.make_psdus without its per-frame Python loop for the header: same header and payload, FCS by zlib per frame"""
    import zlib
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.empty((n, length), dtype=np.uint8)
    hdr = np.frombuffer(txgen.mac_frame(b"", seq=0)[:24], dtype=np.uint8)
    out[:, :24] = hdr
    seq = (np.arange(n) & 0xFFF) << 4
    out[:, 22] = seq & 0xFF
    out[:, 23] = seq >> 8
    out[:, 24:length - 4] = rng.integers(0, 256, size=(n, length - 28), dtype=np.uint8)
    crc = np.fromiter((zlib.crc32(row) for row in out[:, :length - 4]), dtype=np.uint32, count=n)
    out[:, length - 4:] = crc.view(np.uint8).reshape(n, 4)
    return out


@pytest.mark.timeout(900)
def test_one_million_distinct_frames(orc):
    """config 2's geometry with every frame its own: PSDUs -> GPU TX -> device channel (20 dB, +-0.037 rad/sample) ->
    demod + decode_mac: all COMPLETE and CRC-ok with their own PSDU; records, decisions, LLRs = the oracle on a subset"""
    p = _vector_psdus(N_BIG, PSDU_LEN, 2025)
    n_sym, nb = txgen.n_sym_for(PSDU_LEN, ENC), txgen.RATE_TABLE[ENC][0]
    flen = txgen.frame_samples(PSDU_LEN, ENC)
    assert flen == 4401
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=nb, device=0)
    d_psdu = rx.alloc(p.nbytes).upload(p)
    tmpl = rx.alloc(N_BIG * flen * 8)
    rx.tx_batch_dev(tmpl.ptr, N_BIG * flen, d_psdu.ptr, ENC, psdu_len=np.full(N_BIG, PSDU_LEN, np.uint32),
                    psdu_stride=PSDU_LEN, row_len=flen)
    iq = rx.alloc(N_BIG * SLOT * 8)
    rx.synth_slots_dev(tmpl.ptr, N_BIG, flen, iq.ptr, SLOT, N_BIG, LEAD, 20.0, 0.037, 777)
    # spot check of the templates against the restatement
    pick_t = np.array([0, 1, 126, 127, 500_000, N_BIG - 1])
    for f in pick_t:
        row = np.empty(flen, np.complex64)
        rx._check(capi.lib().wifirx_memcpy_d2h(rx._h, row.ctypes.data_as(C.c_void_p), tmpl.ptr + int(f) * flen * 8, row.nbytes))
        assert np.array_equal(row, tx_ref.encode(p[f:f + 1], ENC, [int(f) % 127 + 1])[0]), f
    tmpl.free()
    d_psdu.free()
    dev = rx.alloc_out(N_BIG, psdu_stride=304, want_hbits=True)
    rx.demod_batch_dev(iq.ptr, SLOT, N_BIG, dev)
    rx.decode_batch_dev(N_BIG, dev)
    rx.sync()
    fr = dev["frames"].download(capi.FRAME_DTYPE, N_BIG)
    assert ((fr["flags"] & capi.F_COMPLETE) != 0).all()
    assert ((fr["flags"] & capi.F_CRC_OK) != 0).all(), int(((fr["flags"] & capi.F_CRC_OK) == 0).sum())
    got = dev["psdu"].download(np.uint8, N_BIG * 304).reshape(N_BIG, 304)
    assert np.array_equal(got[:, :PSDU_LEN], p)
    del got
    pick = np.sort(np.random.default_rng(9).choice(N_BIG, SUBSET, replace=False))
    row_i, row_l = n_sym * 48, n_sym * 48 * nb * 4
    lib = capi.lib()

    def rows(buf, f, row_bytes, dtype):
        out = np.empty(row_bytes // np.dtype(dtype).itemsize, dtype=dtype)
        rx._check(lib.wifirx_memcpy_d2h(rx._h, out.ctypes.data_as(C.c_void_p), buf.ptr + int(f) * row_bytes, out.nbytes))
        return out

    x = np.stack([rows(iq, f, SLOT * 8, np.complex64) for f in pick])
    g_idx = np.stack([rows(dev["idx"], f, row_i, np.uint8) for f in pick]).reshape(SUBSET, n_sym, 48)
    g_llr = np.stack([rows(dev["llr"], f, row_l, np.uint32) for f in pick])
    o = orc.demod_batch(x.reshape(-1), SLOT, orc.make_params(max_sym=n_sym, llr_bits=nb), n_threads=min(os.cpu_count() or 1, 16))
    rec = fr[pick].copy()
    rec["flags"] &= ~np.uint32(capi.F_DECODED | capi.F_CRC_OK)
    assert np.array_equal(rec, o["frames"])
    assert np.array_equal(g_idx, o["idx"])
    assert np.array_equal(g_llr.reshape(-1), o["llr"].view(np.uint32).reshape(-1))
    rx.free_out(dev)
    iq.free()
    rx.close()


def _feed_image_through_tx(img):
    from wifirx import app, block, grshim
    tx = block.wifi_phy_tx(encoding=0, pad_front=100, pad_tail=1000)
    pieces = app.detach_image_sorted(img)
    assert len(pieces) == 2700
    for k, piece in enumerate(pieces):
        psdu = np.frombuffer(txgen.mac_frame(app.pack_piece(piece), seq=k), dtype=np.uint8)
        tx._handlers[grshim.intern("mac_in")](grshim.make_pdu({}, psdu))
        if k == 1000:                                    # part of the stream built before the rest has arrived
            yield tx, 1000
    yield tx, None


def test_config5_six_images_through_wifi_phy_tx():
    """the 2700 pieces of each kodim_300 image through wifi_phy_tx (pad 100 / 1000 = IRS_user.py:193) -> x10 + the host AWGN
    of test_config5_six_kodak_images_pixel_exact -> wifi_phy_rx -> extract_pics: pixel-exact; work() buffers both smaller
    than a frame and larger than many"""
    from wifirx import app, block, grshim
    imgs = np.load(os.path.join(GOLD, "kodim_300.npz"))
    assert len(imgs.files) == 6
    for n_img, name in enumerate(sorted(imgs.files)):
        img = imgs[name]
        sizes = (333, 65536) if n_img % 2 == 0 else (100_000, 777)
        parts = []
        for tx, _ in _feed_image_through_tx(img):
            for size in sizes:
                buf = np.empty(size, np.complex64)
                while True:
                    n = tx.work([], [buf])
                    if n == 0:
                        break
                    parts.append(buf[:n].copy())
        assert tx.pending() == 0
        tx.close()
        x = np.concatenate(parts)
        # the same stream as txgen + packet_pad2 builds on the host
        pieces = app.detach_image_sorted(img)
        head = [np.frombuffer(txgen.mac_frame(app.pack_piece(pieces[k]), seq=k), np.uint8) for k in range(3)]
        want = np.concatenate([txgen.packet_pad(txgen.encode_psdus(h[None], 0, [k + 1]).samples, 100, 1000)
                               for k, h in enumerate(head)])
        assert np.abs(x[:want.size] - want).max() <= 1e-6
        x = x * np.float32(10.0)
        rng = np.random.default_rng(sum(name.encode()))
        x += ((rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * np.sqrt(0.5)).astype(np.complex64)
        rx = block.wifi_phy_rx(bandwidth=20e6, frequency=5.89e9, publish_carrier=False)
        got = []
        pics = app.extract_pics(sink=got.append)
        grshim.msg_connect(rx, "mac_out", pics, "MAC")
        grshim.run_stream(rx, x, chunk=8192)
        out = np.zeros_like(img)
        for g in got:
            app.redraw_image(app.load_piece(g), out)
        rx.close()
        assert len(got) == 2700, (name, len(got))
        assert np.array_equal(out, img), name


def test_wifi_phy_tx_seed_and_encoding():
    from wifirx import block
    tx = block.wifi_phy_tx(encoding=3)
    assert tx.get_encoding() == 3
    tx.set_encoding(1)
    p = [rand_psdus(1, 60, k)[0] for k in range(130)]
    for v in p[:129]:
        tx._handlers["mac_in"]((({}), v))
    buf = np.empty(10_000_000, np.complex64)
    n = tx.work([], [buf])
    for v in p[129:]:
        tx._handlers["mac_in"]((({}), v))
    n2 = tx.work([], [buf[n:]])
    f = txgen.frame_samples(60, 1)
    assert n == 129 * f and n2 == f
    stream = buf[:n + n2].reshape(130, f)
    seeds = (np.arange(130) % 127) + 1
    assert np.array_equal(stream, tx_ref.encode(np.stack(p), 1, seeds))
    tx.close()
