"""wifirx_tx_batch_rates, the GPU transmitter with one encoding per frame (wr_tx.hip, tx_kernel<6, true>), through the C ABI
and the block.  Every comparison is exact: row i of a mixed call is what wifirx_tx_batch writes for frame i alone at
encoding[i] with the same seed, i.e. tests/tx_ref.py's encode (NUMERICS.md rule 16, per frame)."""
import ctypes as C

import numpy as np
import pytest

import rates_ref
import tx_ref
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

NAN_WORD = np.uint32(0x7FC0DEAD)

# a few long frames (1 528 bytes at BPSK 1/2 is 511 symbols) among many of one byte: a one-byte frame is 481 samples at every
# encoding but BPSK 1/2 (561), so tight rows put five or six rows of different rates into one 2048-sample tile
LENGTHS = [1, 1528, 24, 100, 1, 1, 1, 1, 1, 1, 1, 294, 1, 700, 57, 1, 1500, 28, 333, 1, 1, 1, 1, 1, 1, 1, 1, 2, 23, 24, 1, 1]
ENCODINGS = [3, 0, 5, 1, 7, 2, 6, 1, 4, 0, 5, 6, 3, 2, 7, 7, 4, 0, 1, 2, 6, 4, 3, 5, 1, 7, 0, 6, 7, 7, 2, 5]


@pytest.fixture(scope="module")
def rx():
    r = capi.WifiRx(max_sym=64, llr_bits=0, device=0)
    yield r
    r.close()


def nan_buf(rx, n_samples):
    buf = rx.alloc(n_samples * 8)
    buf.upload(np.full(n_samples * 2, NAN_WORD, dtype=np.uint32))
    return buf


def mixed_batch(seed=11):
    rng = np.random.default_rng(seed)
    psdus = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in LENGTHS]
    enc = np.array(ENCODINGS, np.uint8)
    assert len(psdus) == enc.size and set(enc.tolist()) == set(range(8))
    seeds = rng.integers(1, 128, enc.size).astype(np.uint8)
    return psdus, enc, seeds, rates_ref.encode_rates(psdus, enc, seeds)


def test_mixed_fixed_rows_bit_exact(rx):
    """host PSDUs of mixed lengths, explicit seeds, fixed rows of odd length: every row = tx_ref.encode of its frame, zeros
    around the frame, canaries around the rows"""
    psdus, enc, seeds, want = mixed_batch()
    n, lead = len(psdus), 37
    for f, p, e in zip(want, psdus, enc):
        assert f.size == txgen.frame_samples(len(p), int(e))
    row = lead + max(f.size for f in want) + 4
    out = nan_buf(rx, n * row + 5)
    rx.tx_batch_dev(out.ptr + 16, n * row, psdus, enc, seeds=seeds, lead=lead, row_len=row)
    got = out.download(np.complex64, n * row + 5)
    out.free()
    assert np.isnan(got[:2]).all() and np.isnan(got[2 + n * row:]).all(), "samples outside the rows were touched"
    rows = got[2:2 + n * row].reshape(n, row)
    assert not np.isnan(rows).any()
    for i, f in enumerate(want):
        assert np.array_equal(rows[i, lead:lead + f.size], f), (i, int(enc[i]), LENGTHS[i])
        assert not rows[i, :lead].any() and not rows[i, lead + f.size:].any(), i
    # the host form: default row length = lead + the longest frame, each at its own encoding
    host = rx.tx_batch(psdus, enc, seeds=seeds, lead=lead)
    assert host.shape == (n, row - 4) and host.tobytes() == rows[:, :row - 4].tobytes()


def test_short_frames_fixed_rows_many_rows_per_tile(rx):
    """one-byte frames at every encoding in fixed rows of 563 samples: four or five rows of different rates per tile"""
    rng = np.random.default_rng(5)
    n, lead = 96, 1
    enc = rng.integers(0, 8, n).astype(np.uint8)
    psdus = [rng.integers(0, 256, 1, dtype=np.uint8).tobytes() for _ in range(n)]
    want = rates_ref.encode_rates(psdus, enc)
    row = lead + 561 + 1
    rows = rx.tx_batch(psdus, enc, lead=lead, row_len=row)
    for i, f in enumerate(want):
        assert f.size == (561 if enc[i] == 0 else 481)
        assert np.array_equal(rows[i, lead:lead + f.size], f), (i, int(enc[i]))
        assert not rows[i, :lead].any() and not rows[i, lead + f.size:].any(), i


@pytest.mark.parametrize("shift", (0, 1))
def test_mixed_row_off_rows_bit_exact(rx, shift):
    """rows of unequal length given by row_off (tight behind the one-byte frames: five or six rows of different rates in a
    tile), the buffer 16 bytes aligned and 8 but not 16 (the kernel's shifted stores)"""
    psdus, enc, seeds, want = mixed_batch(12)
    n = len(psdus)
    lead = 0
    tail = [0 if len(p) == 1 else 3 + (i % 5) for i, p in enumerate(psdus)]
    rows = [lead + f.size + t for f, t in zip(want, tail)]
    row_off = np.concatenate([[7], 7 + np.cumsum(rows)]).astype(np.uint64)
    total = int(row_off[-1])
    out = nan_buf(rx, total + 4)
    rx.tx_batch_dev(out.ptr + 8 * shift, total, psdus, enc, seeds=seeds, lead=lead, row_off=row_off)
    got = out.download(np.complex64, total + 4)[shift:]
    out.free()
    assert np.isnan(got[:7]).all() and np.isnan(got[total:]).all(), "samples outside the rows were touched"
    for i, f in enumerate(want):
        r = got[int(row_off[i]):int(row_off[i + 1])]
        assert np.array_equal(r[lead:lead + f.size], f), (i, int(enc[i]), LENGTHS[i])
        assert not r[:lead].any() and not r[lead + f.size:].any(), i


def test_equal_to_eight_single_encoding_calls(rx):
    """the same frames through eight wifirx_tx_batch calls, one per encoding: the same rows byte for byte; a uniform encoding[]
    through the new entry point = wifirx_tx_batch"""
    psdus, enc, seeds, want = mixed_batch(13)
    lead = 20
    row = lead + max(f.size for f in want)
    mixed = rx.tx_batch(psdus, enc, seeds=seeds, lead=lead, row_len=row)
    for e in range(8):
        sel = np.nonzero(enc == e)[0]
        single = rx.tx_batch([psdus[i] for i in sel], e, seeds=seeds[sel], lead=lead, row_len=row)
        assert single.tobytes() == mixed[sel].tobytes(), e
        sub = [psdus[i] for i in sel]
        uniform = rx.tx_batch(sub, np.full(sel.size, e, np.uint8), seeds=seeds[sel], lead=lead, row_len=row)
        assert uniform.tobytes() == single.tobytes(), e


def test_argument_errors_launch_nothing(rx):
    lib = capi.lib()
    rng = np.random.default_rng(1)
    p = rng.integers(0, 256, (4, 100), dtype=np.uint8)
    lens = np.full(4, 100, np.uint32)
    enc = np.array([7, 6, 5, 4], np.uint8)
    f4 = txgen.frame_samples(100, 4)                      # the longest of the four
    row = f4 + 10
    n_s = 4 * row + 64
    out = nan_buf(rx, n_s)
    canary = out.download(np.uint8, n_s * 8)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(e=enc, n=4, row_len=row, lead=0, row_off=None, h=rx._h):
        return lib.wifirx_tx_batch_rates(h, P(e), P(p), 0, 100, P(lens), None, n, out.ptr, n_s, P(row_off), row_len, lead)

    assert call(e=None) == capi.EINVAL
    assert call(e=np.array([7, 6, 8, 4], np.uint8)) == capi.EINVAL
    assert call(e=np.array([7, 255, 5, 4], np.uint8)) == capi.EINVAL
    assert call(h=None) == capi.EINVAL
    # the row holds a frame at 64-QAM 3/4 but not at BPSK 1/2, which is what frame 3 is given
    slow = np.array([7, 7, 7, 0], np.uint8)
    assert txgen.frame_samples(100, 7) <= row < txgen.frame_samples(100, 0)
    assert call(e=slow) == capi.ERANGE
    f7 = txgen.frame_samples(100, 7)
    assert call(e=slow, row_len=0, row_off=np.array([0, f7, 2 * f7, 3 * f7, 4 * f7], np.uint64)) == capi.ERANGE
    assert call(lead=11) == capi.ERANGE                   # frame 3 (16-QAM 1/2) plus lead no longer fits
    assert call(n=0, e=None) == capi.OK
    rx.sync()
    assert out.download(np.uint8, n_s * 8).tobytes() == canary.tobytes(), "a refused call wrote samples"
    assert call() == capi.OK
    rx.sync()
    got = out.download(np.complex64, n_s)[:4 * row].reshape(4, row)
    out.free()
    for i in range(4):
        f = txgen.frame_samples(100, int(enc[i]))
        assert np.array_equal(got[i, :f], tx_ref.encode(p[i:i + 1], int(enc[i]), [i + 1])[0]), i
        assert not got[i, f:].any()


def test_noiseless_loopback_mixed_batch():
    """8 x 512 MAC frames, lengths drawn per frame, encodings shuffled, rows by row_off -> demod + decode_mac: every frame
    COMPLETE and CRC-ok at its own encoding, its PSDU back, its decisions = txgen's data_idx"""
    rng = np.random.default_rng(77)
    n, lead, tail = 8 * 512, 160, 240
    enc = rng.permutation(np.repeat(np.arange(8, dtype=np.uint8), 512))
    plen = rng.integers(0, 1501, n).astype(np.uint32)
    plen[:16] = np.repeat([0, 1500], 8)                    # both ends of the range at every encoding
    enc[:16] = np.tile(np.arange(8, dtype=np.uint8), 2)
    L = plen + 28
    max_sym = max(txgen.n_sym_for(int(l), int(e)) for l, e in zip(L, enc))
    assert max_sym == txgen.n_sym_for(1528, 0) == 511
    rx = capi.WifiRx(max_sym=max_sym, llr_bits=0, device=0)
    psdu = rx.mac_batch(n, None, payload_len=plen, payload_seed=3)
    stride = psdu.shape[1]
    rows = np.array([lead + txgen.frame_samples(int(l), int(e)) + tail for l, e in zip(L, enc)], np.uint64)
    rows += rows & np.uint64(1)
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint64)
    total = int(row_off[-1])
    d_psdu = rx.alloc(psdu.nbytes).upload(psdu)
    iq = rx.alloc(total * 8)
    dev = rx.alloc_out(n, psdu_stride=1536)
    try:
        rx.tx_batch_dev(iq.ptr, total, d_psdu.ptr, enc, psdu_len=L, psdu_stride=stride, lead=lead, row_off=row_off)
        rx.demod_batch_var_dev(iq.ptr, row_off, dev)
        rx.decode_batch_dev(n, dev)
        rx.sync()
        r = rx.download_out(dev, n)
    finally:
        rx.free_out(dev)
        iq.free()
        d_psdu.free()
        rx.close()
    fr = r["frames"]
    want_flags = capi.F_COMPLETE | capi.F_CRC_OK
    assert ((fr["flags"] & want_flags) == want_flags).all(), int(((fr["flags"] & want_flags) != want_flags).sum())
    assert np.array_equal(fr["encoding"], enc)
    assert np.array_equal(fr["psdu_len"], L)
    for i in range(n):
        li, e = int(L[i]), int(enc[i])
        assert np.array_equal(r["psdu"][i, :li], psdu[i, :li]), i
        tx = txgen.encode_psdus(psdu[i:i + 1, :li], e, [i % 127 + 1])
        assert fr["n_sym"][i] == tx.n_sym
        assert np.array_equal(r["idx"][i, :tx.n_sym], tx.data_idx[0]), (i, e, li)


def test_wifi_phy_tx_applies_the_encoding_in_force_at_each_pdu():
    """PDUs interleaved with set_encoding before one work(): each frame at the rate in force when its PDU arrived"""
    from wifirx import block
    rng = np.random.default_rng(4)
    tx = block.wifi_phy_tx(encoding=2, pad_front=3, pad_tail=5)
    plan = [(None, 60), (None, 1), (7, 200), (None, 33), (0, 61), (5, 294), (5, 10), (1, 77), (None, 1), (6, 500), (3, 90), (4, 28)]
    psdus, encs, cur = [], [], 2
    for e, L in plan:
        if e is not None:
            tx.set_encoding(e)
            cur = e
        v = rng.integers(0, 256, L, dtype=np.uint8)
        tx._handlers["mac_in"]((({}), v))
        psdus.append(v.tobytes())
        encs.append(cur)
    tx.set_encoding(0)                                     # after the last PDU: applies to none of them
    buf = np.empty(1_000_000, np.complex64)
    n = tx.work([], [buf])
    # a second work(): the seeds go on counting, the queue is at one rate
    v = rng.integers(0, 256, 40, dtype=np.uint8)
    tx._handlers["mac_in"]((({}), v))
    n2 = tx.work([], [buf[n:]])
    tx.close()
    psdus.append(v.tobytes())
    encs.append(0)
    frames = rates_ref.encode_rates(psdus, encs, np.arange(len(psdus)) % 127 + 1)
    want = np.concatenate([txgen.packet_pad(f[None], 3, 5) for f in frames])
    assert n + n2 == want.size and n2 == 3 + frames[-1].size + 5
    assert np.array_equal(buf[:n + n2], want)
