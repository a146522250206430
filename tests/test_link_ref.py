"""The host statements of the loop-back's two ends (tests/link_ref.py) and the mac block, without a GPU:
  * link_ref.mac_batch == txgen.mac_frame frame by frame (lengths, sequence wrap, addresses), CRC residue, txgen.make_psdus;
    its Philox payload == channel_ref.philox4x32_10 word by word;
  * link_ref.link_stats on hand-made records of every class gives the counts written out here; hbits and idx forms agree;
  * block.mac: `app in` -> `phy out` -> wifi_phy_tx.mac_in, PSDU = txgen.mac_frame, the sequence number counts up, and the
    reference's consumer slice gives back the bytes behind its 4-byte prefix."""
import struct
import zlib

import numpy as np
import pytest

import channel_ref
import link_ref
from wifirx import txgen

LENGTHS = (0, 1, 3, 262, 266, 1500)
ADDR = (bytes([0x10, 0x22, 0x33, 0x44, 0x55, 0x66]), bytes(range(1, 7)), bytes([0xAA, 0xBB, 0xCC, 0xDD, 0xEE, 0x0F]))   # dst, src, bss
CRC_RESIDUE = 0x2144DF1C


def frames_by_mac_frame(payloads, seq0=0, addr=None):
    kw = {} if addr is None else dict(dst=addr[0], src=addr[1], bss=addr[2])
    return [txgen.mac_frame(bytes(p), seq=seq0 + k, **kw) for k, p in enumerate(payloads)]


@pytest.mark.parametrize("length", LENGTHS)
def test_mac_batch_is_mac_frame(length):
    rng = np.random.default_rng(length)
    n = 9
    pay = rng.integers(0, 256, (n, length), dtype=np.uint8)
    for seq0, addr in ((0, None), (0xFFA, None), (5, ADDR), (0x12345FFE, ADDR)):     # 0xFFA + 8 crosses 0xFFF
        got = link_ref.mac_batch(n, pay, seq0=seq0, addr=addr)
        want = frames_by_mac_frame(pay, seq0, addr)
        assert [bytes(g) for g in got] == want
        for g in got:
            assert len(g) == 28 + length
            assert zlib.crc32(bytes(g)) == CRC_RESIDUE


def test_mac_batch_mixed_lengths_and_lists():
    rng = np.random.default_rng(7)
    lens = [LENGTHS[k % len(LENGTHS)] for k in range(13)]
    pays = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in lens]
    assert [bytes(g) for g in link_ref.mac_batch(13, pays, seq0=0xFF8)] == frames_by_mac_frame(pays, 0xFF8)
    wide = np.zeros((13, 1500), np.uint8)
    for k, p in enumerate(pays):
        wide[k, :len(p)] = np.frombuffer(p, np.uint8)
    assert [bytes(g) for g in link_ref.mac_batch(13, wide, payload_len=lens, seq0=0xFF8)] == frames_by_mac_frame(pays, 0xFF8)


def test_mac_batch_reproduces_make_psdus():
    for n, plen, seed, seq0 in ((5, 294, 2025, 0), (3, 28, 1, 4094), (4, 100, 9, 17)):
        want = txgen.make_psdus(n, plen, seed=seed, seq0=seq0)
        pay = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(n, plen - 28), dtype=np.uint8)
        got = link_ref.mac_batch(n, pay, seq0=seq0)
        assert np.array_equal(np.stack(got), want)


def test_philox_payload_word_by_word():
    seed = 0x0123456789ABCDEF
    n, length = 5, 266
    pay = link_ref.philox_payload(n, length, seed)
    assert pay.shape == (n, length)
    for i in range(n):
        for j in range((length + 15) // 16):
            w = channel_ref.philox4x32_10([j], [i], [0], [0], seed & 0xFFFFFFFF, seed >> 32)
            blk = b"".join(struct.pack("<I", int(v[0])) for v in w)
            assert pay[i, 16 * j:16 * j + 16].tobytes() == blk[:min(16, length - 16 * j)], (i, j)
    # a longer payload starts with the shorter one; another seed gives other bytes; the PSDUs carry it
    assert np.array_equal(link_ref.philox_payload(n, 300, seed)[:, :length], pay)
    assert not np.array_equal(link_ref.philox_payload(n, length, seed + 1), pay)
    got = link_ref.mac_batch(n, None, payload_len=length, seq0=3, payload_seed=seed)
    assert [bytes(g) for g in got] == frames_by_mac_frame(pay, 3)
    mixed = link_ref.mac_batch(n, None, payload_len=[0, 1, 3, 262, 266], payload_seed=seed)
    assert [bytes(g) for g in mixed] == frames_by_mac_frame([pay[k, :L] for k, L in enumerate((0, 1, 3, 262, 266))])


def test_crc32_rows_is_zlib():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 256, (20, 90), dtype=np.uint8)
    lens = rng.integers(0, 91, 20)
    got = link_ref.crc32_rows(rows, lens)
    assert [int(c) for c in got] == [zlib.crc32(rows[k, :lens[k]].tobytes()) for k in range(20)]


# ---- link_stats ----

ENC = [7, 0, 2, 4, 6, 1, 3, 5]
N_SYM = [2, 1, 3, 2, 3, 1, 2, 3]


def test_link_stats_every_class():
    """one frame per class, in the order of link_ref.CLASSES; good frames: 4 (64-QAM, 3 symbols: 864 bits), 5 (BPSK, 1: 48),
    6 (QPSK, 2: 192, one bit wrong), 7 (16-QAM, 3: 576, all wrong)"""
    rng = np.random.default_rng(11)
    rx, ref = link_ref.hand_made_batch(rng, range(8), ENC, N_SYM, max_sym=3)
    want = dict(frames=8, frames_ref=7, frames_good=4, frames_crc_ok=3, frames_psdu_ok=1, frames_crc_ok_wrong=2,
                coded_bits=864 + 48 + 192 + 576, coded_bit_errors=1 + 576, coded_bit_errors_sq=1 + 576 * 576)
    M = 0xFFFFFFFF
    for use_hbits in (True, False):
        counts, err, cls = link_ref.link_stats(rx, ref, 3, use_hbits=use_hbits)
        assert counts == want, use_hbits
        assert err.tolist() == [M, M, M, M, 0, 0, 1, 576]
        #                      ref_inc rx_inc  enc  len   flipped  equal      1 bit  all
        assert cls.tolist() == [0,     8,      8,   8 | 2, 8 | 2 | 1, 8 | 4 | 2 | 1, 8 | 1, 8 | 1]
    # without the PSDUs the three PSDU counters stay 0; without the decisions the three coded-bit counters do
    no_psdu = dict(ref, psdu=None)
    counts, err, cls = link_ref.link_stats(rx, no_psdu, 3)
    assert counts == dict(want, frames_crc_ok=0, frames_psdu_ok=0, frames_crc_ok_wrong=0)
    assert cls.tolist() == [0, 8, 8, 8, 9, 9, 9, 9]
    no_dec = dict(ref, idx=None, hbits=None)
    counts, err, cls = link_ref.link_stats(rx, no_dec, 3)
    assert counts == dict(want, coded_bits=0, coded_bit_errors=0, coded_bit_errors_sq=0)
    assert (err == M).all()
    # hbits on one side only: the idx form is used
    counts, err, _ = link_ref.link_stats(rx, dict(ref, hbits=None), 3)
    assert counts == want and err.tolist()[4:] == [0, 0, 1, 576]


def test_link_stats_hbits_and_idx_agree_shuffled():
    rng = np.random.default_rng(12)
    n, max_sym = 400, 5
    classes = rng.integers(0, 8, n)
    rx, ref = link_ref.hand_made_batch(rng, classes, rng.integers(0, 8, n), rng.choice([1, max_sym], n), max_sym)
    a = link_ref.link_stats(rx, ref, max_sym, use_hbits=True)
    b = link_ref.link_stats(rx, ref, max_sym, use_hbits=False)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[0]["frames_ref"] == n - int((classes == 0).sum())
    assert a[0]["frames_good"] == int((classes >= 4).sum())
    assert a[0]["frames_psdu_ok"] == int((classes == 5).sum())
    assert a[0]["frames_crc_ok_wrong"] == int(((classes == 3) | (classes == 4)).sum())
    assert a[0]["coded_bit_errors"] > 0 and a[0]["coded_bits"] > 0
    # a record that claims more symbols than the rows hold is not good (nothing behind a row is read)
    rx["frames"]["n_sym"][:] = max_sym + 1
    ref["frames"]["n_sym"][:] = max_sym + 1
    assert link_ref.link_stats(rx, ref, max_sym, use_hbits=False)[0]["frames_good"] == 0


# ---- the mac block ----

def test_mac_block_through_the_shim():
    from wifirx import block, grshim
    rng = np.random.default_rng(5)
    m = block.mac(ADDR[1], ADDR[0], ADDR[2])                      # (src, dst, bss): the argument order of ieee802_11.mac
    got = []
    grshim.msg_connect(m, grshim.intern("phy out"), grshim.sink_block(got.append), "in")
    payloads = [struct.pack("=L", k) + rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes() for k in range(7)]
    for p in payloads:
        m._handlers[grshim.intern("app in")](grshim.make_pdu({}, np.frombuffer(p, np.uint8)))
    assert len(got) == 7
    for k, (meta, vec) in enumerate(got):
        psdu = bytes(np.asarray(vec, np.uint8))
        assert psdu == txgen.mac_frame(payloads[k], seq=k, src=ADDR[1], dst=ADDR[0], bss=ADDR[2])
        assert zlib.crc32(psdu) == CRC_RESIDUE
        # wifi_phy_rx publishes the PSDU without its FCS on mac_out; the reference's consumer (IRS_AP_epy_block_2.py:31-36)
        # takes [24:] of it, and [4:] of that is the data behind the 4-byte counter
        data = psdu[:-4][24:]
        assert struct.unpack("=L", data[:4])[0] == k and data[4:] == payloads[k][4:]
    # default addresses are the reference's (gnu_radio/IRS_user.py:192)
    d = block.mac()
    out = []
    grshim.msg_connect(d, "phy out", grshim.sink_block(out.append), "in")
    d._handlers["app in"](({}, np.zeros(3, np.uint8)))
    assert bytes(out[0][1]) == txgen.mac_frame(bytes(3), seq=0)
    with pytest.raises(ValueError):
        d._handlers["app in"](({}, np.zeros(1501, np.uint8)))
    with pytest.raises(ValueError):
        block.mac(src_mac=(1, 2, 3))


def test_mac_block_wires_into_wifi_phy_tx():
    """`phy out` -> wifi_phy_tx.mac_in: the PDU is taken as it is (the handle-free part: the queue of PSDUs)"""
    from wifirx import block, grshim

    class tx_stub(grshim.basic_block):                            # wifi_phy_tx's message side without a device
        def __init__(self):
            grshim.basic_block.__init__(self, name="wifi_phy_tx")
            self._queue = []
            self.message_port_register_in(grshim.intern("mac_in"))
            self.set_msg_handler(grshim.intern("mac_in"), lambda msg: block.wifi_phy_tx._on_pdu(self, msg))

    m, tx = block.mac(), tx_stub()
    grshim.msg_connect(m, "phy out", tx, "mac_in")
    for k in range(3):
        m._handlers["app in"](({}, np.full(10 + k, k, np.uint8)))
    assert tx._queue == [txgen.mac_frame(bytes([k]) * (10 + k), seq=k) for k in range(3)]
