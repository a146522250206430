"""Host statement (vectorised NumPy) of the two ends of the device loop-back, the reference of the tests:
  * mac_batch  = wifirx_mac_batch: ieee802_11.mac's PSDUs (24-byte data header, payload, CRC-32) for a batch, with the
    Philox payload of include/wifirx.h when none is given;
  * link_stats = wifirx_link_stats: the nine counters, frame_err and frame_class of a decoded batch against what was sent;
  * pack_hbits = the bit planes of include/wifirx.h (wifirx_out.hbits) of `idx` rows."""
import numpy as np

import channel_ref

F_COMPLETE, F_CRC_OK = 0x08, 0x40
N_BPSC = np.array([1, 1, 2, 2, 4, 4, 6, 6])
DATA_BINS = np.array([i for i in range(6, 59) if i not in (11, 25, 32, 39, 53)])       # data carrier c -> FFT bin (shifted)
MAX_PAYLOAD = 1500
COUNTERS = ("frames", "frames_ref", "frames_good", "frames_crc_ok", "frames_psdu_ok", "frames_crc_ok_wrong", "coded_bits",
            "coded_bit_errors", "coded_bit_errors_sq")
POPCOUNT8 = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def _crc_table():
    c = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        c = (c >> np.uint32(1)) ^ (np.uint32(0xEDB88320) * (c & np.uint32(1)))
    return c


CRC_TABLE = _crc_table()


def crc32_rows(rows, lens):
    """CRC-32 (reflected 0xEDB88320, as zlib.crc32) of rows[i, :lens[i]]: the byte-wise table form, all rows in step"""
    rows = np.asarray(rows, np.uint8)
    lens = np.asarray(lens, np.int64)
    crc = np.full(rows.shape[0], 0xFFFFFFFF, np.uint32)
    for p in range(int(lens.max(initial=0))):
        act = lens > p
        crc[act] = (crc[act] >> np.uint32(8)) ^ CRC_TABLE[(crc[act] ^ rows[act, p]) & np.uint32(0xFF)]
    return ~crc


def philox_payload(n_frames, length, seed, first_frame=0):
    """[n_frames, length] uint8: bytes 16 j .. 16 j + 15 of frame i = the words x, y, z, w (little endian) of
    philox4x32_10((j, i, 0, 0), (seed & 0xffffffff, seed >> 32))"""
    n_blk = (length + 15) // 16
    if n_frames == 0 or n_blk == 0:
        return np.zeros((n_frames, length), np.uint8)
    i, j = np.meshgrid(np.arange(first_frame, first_frame + n_frames, dtype=np.uint32), np.arange(n_blk, dtype=np.uint32),
                       indexing="ij")
    z = np.zeros_like(i)
    w = channel_ref.philox4x32_10(j, i, z, z, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=-1).astype("<u4")                      # [n, n_blk, 4]
    return np.ascontiguousarray(words).view(np.uint8).reshape(n_frames, n_blk * 16)[:, :length].copy()


def mac_batch(n_frames, payload=None, payload_len=None, seq0=0, addr=None, payload_seed=0):
    """List of n_frames PSDUs (uint8 arrays).  payload: None (Philox), a 2-D uint8 array or a list of bytes; payload_len: one
    length or [n_frames], default the width of `payload`; addr = (dst, src, bss)."""
    n = int(n_frames)
    if payload is not None and not isinstance(payload, np.ndarray):
        if payload_len is None:
            payload_len = [len(p) for p in payload]
        arr = np.zeros((n, max(max((len(p) for p in payload), default=0), 1)), np.uint8)
        for k, p in enumerate(payload):
            arr[k, :len(p)] = np.frombuffer(bytes(p), np.uint8)
        payload = arr
    if payload_len is None:
        payload_len = payload.shape[1]
    lens = np.broadcast_to(np.asarray(payload_len, np.int64), (n,))
    assert (lens >= 0).all() and (lens <= MAX_PAYLOAD).all()
    width = int(lens.max(initial=0))
    pay = philox_payload(n, width, int(payload_seed)) if payload is None else np.asarray(payload, np.uint8)[:, :width]
    dst, src, bss = ((0x42,) * 6, (0x23,) * 6, (0xFF,) * 6) if addr is None else addr
    rows = np.zeros((n, 24 + width + 4), np.uint8)
    rows[:, 0] = 0x08
    rows[:, 4:10], rows[:, 10:16], rows[:, 16:22] = (np.frombuffer(bytes(bytearray(a)), np.uint8) for a in (dst, src, bss))
    seq = ((int(seq0) + np.arange(n, dtype=np.int64)) & 0xFFF) << 4
    rows[:, 22], rows[:, 23] = seq & 0xFF, seq >> 8
    rows[:, 24:24 + width] = pay
    crc = crc32_rows(rows, 24 + lens)
    out = []
    for k in range(n):
        body = 24 + int(lens[k])
        out.append(np.concatenate([rows[k, :body], np.array([int(crc[k]) >> s & 0xFF for s in (0, 8, 16, 24)], np.uint8)]))
    return out


def mac_rows(psdus, stride, fill=0):
    """the PSDUs of mac_batch as rows of `stride` bytes, `fill` behind each"""
    out = np.full((len(psdus), stride), fill, np.uint8)
    for k, p in enumerate(psdus):
        out[k, :len(p)] = p
    return out


def pack_hbits(frames, idx, max_sym):
    """wifirx_out.hbits of `idx` ([n, max_sym, 48]): word 2 b + h of data symbol q of a frame with n_bpsc bits per carrier, at
    q * 2 * n_bpsc + 2 b + h of its row of max_sym * 12 words, holds bit b of the FFT bins 32 h .. 32 h + 31"""
    n = len(frames)
    idx = np.asarray(idx, np.uint8).reshape(n, max_sym, 48)
    out = np.zeros((n, max_sym * 12), np.uint32)
    for f in range(n):
        enc = int(frames["encoding"][f])
        n_sym = int(frames["n_sym"][f])
        if enc > 7 or n_sym > max_sym:
            continue
        nb = int(N_BPSC[enc])
        bits = np.zeros((n_sym, nb, 64), np.uint64)
        bits[:, :, DATA_BINS] = (idx[f, :n_sym, None, :] >> np.arange(nb, dtype=np.uint8)[None, :, None]) & 1
        w = (bits << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)                # [n_sym, nb]
        pair = np.stack([w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)], axis=-1).astype(np.uint32)
        out[f, :n_sym * 2 * nb] = pair.reshape(-1)
    return out


def link_stats(rx, ref, max_sym, use_hbits=None):
    """rx, ref: dicts of host arrays -- "frames" (FRAME_DTYPE), optionally "psdu" [n, stride], "idx" [n, max_sym, 48], "hbits"
    [n, max_sym * 12].  Returns (counts dict, frame_err uint32 [n], frame_class uint8 [n]).  The decisions are taken from
    hbits when both sides have them, else from idx (use_hbits overrides).  Vectorised over the frames of one PSDU length
    (the byte comparison) and of one rate and symbol count (the popcount)."""
    fr, ff = rx["frames"], ref["frames"]
    n = len(fr)
    both = lambda k: rx.get(k) is not None and ref.get(k) is not None
    ref_c = (ff["flags"] & F_COMPLETE) != 0
    good = (ref_c & ((fr["flags"] & F_COMPLETE) != 0) & (fr["encoding"] == ff["encoding"]) & (fr["encoding"] < 8)
            & (fr["psdu_len"] == ff["psdu_len"]) & (fr["n_sym"] == ff["n_sym"]) & (fr["n_sym"] <= max_sym))
    crc_ok = ref_c & ((fr["flags"] & F_CRC_OK) != 0) & both("psdu")
    psdu_ok = np.zeros(n, bool)
    if both("psdu"):
        p, q = rx["psdu"], ref["psdu"]
        cand = crc_ok & (fr["psdu_len"] == ff["psdu_len"]) & (fr["psdu_len"] <= min(p.shape[1], q.shape[1]))
        for L in np.unique(fr["psdu_len"][cand]):
            sel = np.nonzero(cand & (fr["psdu_len"] == L))[0]
            psdu_ok[sel] = (p[sel, :int(L)] == q[sel, :int(L)]).all(axis=1)
    if use_hbits is None:
        use_hbits = both("hbits")
    key = "hbits" if use_hbits else "idx"
    err = np.full(n, 0xFFFFFFFF, np.uint32)
    bits = 0
    if both(key):
        a = np.ascontiguousarray(rx[key]).reshape(n, -1).view(np.uint8)          # rows of max_sym * 48 bytes in both forms
        b = np.ascontiguousarray(ref[key]).reshape(n, -1).view(np.uint8)
        for enc, n_sym in sorted(set(zip(fr["encoding"][good].tolist(), fr["n_sym"][good].tolist()))):
            sel = np.nonzero(good & (fr["encoding"] == enc) & (fr["n_sym"] == n_sym))[0]
            nb = int(N_BPSC[enc])
            width = (8 * nb if use_hbits else 48) * n_sym                        # bytes of the row the frame fills
            err[sel] = POPCOUNT8[a[sel, :width] ^ b[sel, :width]].sum(axis=1, dtype=np.uint32)
            bits += sel.size * n_sym * 48 * nb
    e = [int(v) for v in err[good]] if both(key) else []
    counts = dict(frames=n, frames_ref=int(ref_c.sum()), frames_good=int(good.sum()), frames_crc_ok=int(crc_ok.sum()),
                  frames_psdu_ok=int(psdu_ok.sum()), frames_crc_ok_wrong=int((crc_ok & ~psdu_ok).sum()), coded_bits=bits,
                  coded_bit_errors=sum(e), coded_bit_errors_sq=sum(v * v for v in e))
    cls = (good.astype(np.uint8) | (crc_ok.astype(np.uint8) << 1) | (psdu_ok.astype(np.uint8) << 2)
           | (ref_c.astype(np.uint8) << 3))
    return counts, err, cls


# ---- hand-made batches that hit every class of link_stats (tests/test_link_ref.py, tests/test_gpu_link.py) ----

CLASSES = ("ref_incomplete", "rx_incomplete", "other_encoding", "other_length", "crc_ok_byte_flipped", "crc_ok_equal",
           "good_one_bit_wrong", "good_all_bits_wrong")


def hand_made_batch(rng, classes, enc, n_sym, max_sym, rx_stride=64, ref_stride=60, frame_dtype=None):
    """One frame per entry of `classes` (indices into CLASSES) with encoding enc[f] and n_sym[f] data symbols: the reference
    side (records, PSDUs, idx, hbits of what was "sent") and a received side that differs from it by what the class says.
    Everything a frame does not fill -- PSDU bytes behind psdu_len, decisions behind n_sym -- is random and different on
    the two sides: it must not count.  Returns (rx, ref) dicts of host arrays."""
    from wifirx import capi
    dt = frame_dtype or capi.FRAME_DTYPE
    classes, enc, n_sym = (np.asarray(v, np.int64) for v in (classes, enc, n_sym))
    n = classes.size
    nb = N_BPSC[enc]
    L = rng.integers(4, min(rx_stride, ref_stride) + 1, n)
    ref_fr = np.zeros(n, dt)
    ref_fr["flags"] = 0x0F
    ref_fr["trigger"] = 176
    ref_fr["psdu_len"], ref_fr["encoding"], ref_fr["n_bpsc"], ref_fr["n_sym"], ref_fr["n_sym_out"] = L, enc, nb, n_sym, n_sym
    rx_fr = ref_fr.copy()
    rx_fr["flags"] |= 0x20                                           # decode_mac ran
    ref_psdu = rng.integers(0, 256, (n, ref_stride), dtype=np.uint8)
    rx_psdu = rng.integers(0, 256, (n, rx_stride), dtype=np.uint8)
    ref_idx = (rng.integers(0, 64, (n, max_sym, 48)) & ((1 << nb) - 1)[:, None, None]).astype(np.uint8)
    rx_idx = ref_idx.copy()
    for f in range(n):
        rx_psdu[f, :L[f]] = ref_psdu[f, :L[f]]
        rx_idx[f, n_sym[f]:] ^= rng.integers(1, 64, (max_sym - n_sym[f], 48), dtype=np.uint8)
        c = CLASSES[classes[f]]
        if c == "ref_incomplete":
            ref_fr["flags"][f] &= ~np.uint32(F_COMPLETE)
            rx_fr["flags"][f] |= F_CRC_OK
        elif c == "rx_incomplete":
            rx_fr["flags"][f] = 0x01
        elif c == "other_encoding":
            rx_fr["encoding"][f] = (enc[f] + 1) % 8
            rx_fr["n_bpsc"][f] = N_BPSC[rx_fr["encoding"][f]]
        elif c == "other_length":
            rx_fr["psdu_len"][f] = L[f] - 1
            rx_fr["flags"][f] |= F_CRC_OK
        elif c == "crc_ok_byte_flipped":
            rx_fr["flags"][f] |= F_CRC_OK
            rx_psdu[f, rng.integers(0, L[f])] ^= np.uint8(1 << rng.integers(0, 8))
        elif c == "crc_ok_equal":
            rx_fr["flags"][f] |= F_CRC_OK
        elif c == "good_one_bit_wrong":
            rx_idx[f, rng.integers(0, n_sym[f]), rng.integers(0, 48)] ^= np.uint8(1 << rng.integers(0, nb[f]))
        elif c == "good_all_bits_wrong":
            rx_idx[f, :n_sym[f]] ^= np.uint8((1 << nb[f]) - 1)
    rx = dict(frames=rx_fr, psdu=rx_psdu, idx=rx_idx, hbits=pack_hbits(rx_fr, rx_idx, max_sym))
    ref = dict(frames=ref_fr, psdu=ref_psdu, idx=ref_idx, hbits=pack_hbits(ref_fr, ref_idx, max_sym))
    for f in range(n):          # words behind a frame's last symbol are not written by the demodulator: anything may be there
        used = 2 * int(N_BPSC[rx_fr["encoding"][f]]) * int(n_sym[f])
        rx["hbits"][f, used:] = rng.integers(0, 1 << 32, max_sym * 12 - used, dtype=np.uint32)
        used = 2 * int(nb[f]) * int(n_sym[f])
        ref["hbits"][f, used:] = rng.integers(0, 1 << 32, max_sym * 12 - used, dtype=np.uint32)
    return rx, ref
