"""Stream-mode receive diversity on the device: wifirx_detect_multi against the restatement of NUMERICS.md rule 24
(tests/detect_multi_ref.py) bit for bit, and wifirx_push_diversity / wifirx_poll_diversity -- one antenna against wifirx_push
byte for byte, identical and all-zero antennas, independence of chunking / batching / input side / sample format, the
regrowth of three partly filled planes, the end-to-end gain at the operating point of tests/stream_diversity_point.py, the
all-or-nothing contract (float and integer host input), a failure behind the
commit of a pass (WIFIRX_EDEAD), every refused argument, and the wifi_phy_rx block with two input ports."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest

import convert_ref as cr
import detect_multi_ref as mr
import stream_diversity_point as pt
import stream_diversity_rows as sdr
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

KEYS = ("frames", "psdu", "idx", "carrier", "csi", "sym_stats")
THR, MP = 0.56, 2
CHUNKS = (777, 4096, 0)            # 0: the whole stream in one push


# ---- 1. the joint detection kernel ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def joint_reference(n_ant):
    xs = sdr.capture(n_ant)
    Ar, Ai, P = mr.window_sums(xs)
    return Ar, Ai, P, mr.masks(mr.bits(xs, THR))


@pytest.mark.parametrize("want_p", [False, True], ids=["P null", "P given"])
@pytest.mark.parametrize("n_ant", [1, 2, 3, 8])
def test_detect_multi_equals_the_restatement_bit_for_bit(n_ant, want_p):
    xs = sdr.capture(n_ant)
    n = xs[0].size
    assert n == 2 * 4096 + 3 * 64 + 37 == 8421
    Ar, Ai, P, masks = joint_reference(n_ant)
    n_words, pad = (n + 63) // 64, 16
    rx = capi.WifiRx(max_sym=1)
    bufs = []
    try:
        d_x = [rx.alloc(x.nbytes).upload(x) for x in xs]
        s_masks = np.full(n_words + pad, 0xA5A5A5A5A5A5A5A5, np.uint64)
        s_A = np.full(2 * (n + pad), np.float32(-777.25), np.float32)
        s_P = np.full(n + pad, np.float32(-333.5), np.float32)
        d_m, d_A, d_P = rx.alloc(s_masks.nbytes).upload(s_masks), rx.alloc(s_A.nbytes).upload(s_A), rx.alloc(s_P.nbytes).upload(s_P)
        bufs = d_x + [d_m, d_A, d_P]
        rx.detect_multi_dev([d.ptr for d in d_x], n, THR, d_m.ptr, d_A.ptr, d_P.ptr if want_p else None)
        rx.sync()
        g_m, g_A, g_P = d_m.download(np.uint64, s_masks.size), d_A.download(np.float32, s_A.size), d_P.download(np.float32, s_P.size)
    finally:
        for b in bufs:
            b.free()
        rx.close()
    assert np.array_equal(g_m[:n_words], masks), np.flatnonzero(g_m[:n_words] != masks)[:8]
    assert masks.any() and (g_m[n_words - 1] >> np.uint64(n - 64 * (n_words - 1))) == 0        # no bit at or behind n
    A = g_A[:2 * n].reshape(-1, 2)
    assert np.array_equal(A[:, 0].view(np.uint32), Ar.view(np.uint32)) and np.array_equal(A[:, 1].view(np.uint32), Ai.view(np.uint32))
    if want_p:
        assert np.array_equal(g_P[:n].view(np.uint32), P.view(np.uint32))
    else:
        assert np.array_equal(g_P, s_P)
    # the sentinels behind n and behind the last mask word
    assert np.array_equal(g_m[n_words:], s_masks[n_words:]) and np.array_equal(g_A[2 * n:], s_A[2 * n:]) and np.array_equal(g_P[n:], s_P[n:])


# ---- the stream runs -----------------------------------------------------------------------------------------------------------

def new_handle(batch=0, soft=0, max_sym=511):
    rx = capi.WifiRx(max_sym=max_sym, want_carrier=True)
    rx.set_param(capi.P_STREAM_BATCH, batch)
    rx.set_param(capi.P_STREAM_SOFT, soft)
    return rx


def cuts(n, chunk):
    return [(a, min(a + chunk, n)) for a in range(0, n, chunk or n)] if chunk else [(0, n)]


def collect(rx, got, keys):
    out = {k: np.concatenate([g[k] for g in got]) for k in keys}
    out["stats"] = rx.stats()
    return out


@functools.lru_cache(maxsize=None)
def single_run(key, chunk=0, soft=0):
    """the stream `key` (see streams()) through wifirx_push on a handle of its own"""
    x = streams(key)[0]
    rx = new_handle(soft=soft)
    try:
        got = []
        for a, b in cuts(x.size, chunk):
            rx.push(x[a:b])
            got.append(rx.poll(cap=64, want_idx=True, want_csi=True, want_stats=True))
        rx.flush()
        got.append(rx.poll(cap=64, want_idx=True, want_csi=True, want_stats=True))
        return collect(rx, got, KEYS)
    finally:
        rx.close()


def div_run(xs, chunk=0, soft=0, batch=0, mode=capi.DIV_MRC, ant_gain=None, on_device=False, fmt=None, scale=None, edges=None):
    """the antennas' streams xs through wifirx_push_diversity: complex64 arrays, or (with fmt) int16 / int8 arrays [n, 2];
    one push per chunk, or per pair of `edges`"""
    rx = new_handle(batch, soft)
    dev = []
    try:
        got = []
        n = len(xs[0])
        if on_device:
            dev = [rx.alloc(x.nbytes).upload(x) for x in xs]
        item = xs[0].nbytes // n
        for a, b in edges or cuts(n, chunk):
            if on_device:
                rx.push_diversity_dev([d.ptr + a * item for d in dev], b - a, mode, ant_gain, "fc32" if fmt is None else fmt, scale)
            else:
                rx.push_diversity([x[a:b] for x in xs], mode, ant_gain, fmt, scale)
            got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
        rx.flush_diversity(mode, ant_gain)
        got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
        assert rx.queued() == 0
        return collect(rx, got, KEYS + ("used_mask", "ant_frames"))
    finally:
        for d in dev:
            d.free()
        rx.close()


@functools.lru_cache(maxsize=None)
def streams(key):
    """the antennas' streams by name, each a tuple of complex64 arrays"""
    clean, _ = sdr.clean_stream()
    if key == "one":
        return (sdr.antenna(clean, 1.0, 7),)
    if key == "two":            # independent noise and a gain each
        return (sdr.antenna(clean, 1.0, 7), sdr.antenna(clean, 0.7 * np.exp(0.8j), 8))
    raise KeyError(key)


def same_bytes(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), k


# ---- 2. one antenna is the single stream -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("soft", [0, 1], ids=["hard", "soft"])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_one_antenna_equals_wifirx_push(chunk, soft):
    want = single_run("one", chunk, soft)
    got = div_run(streams("one"), chunk, soft)
    assert len(want["frames"]) == 10 and ((want["frames"]["flags"] & capi.F_CRC_OK) != 0).all()
    same_bytes(got, want)
    assert got["stats"] == want["stats"]
    assert (got["used_mask"] == 1).all() and np.array_equal(got["ant_frames"][:, 0]["trigger"], want["frames"]["trigger"])


# ---- 3. identical antennas ---------------------------------------------------------------------------------------------------------

def records_without_llr(fr):
    fr = fr.copy()
    fr["flags"] &= ~np.uint32(capi.F_LLR)
    return fr


def test_two_identical_antennas_mrc():
    x = streams("one")[0]
    want = single_run("one")
    got = div_run((x, x))
    same_bytes(got, want, ("idx", "carrier", "psdu"))
    assert np.array_equal(records_without_llr(got["frames"]), records_without_llr(want["frames"]))
    assert (got["used_mask"] == 3).all() and len(got["used_mask"]) == 10


@pytest.mark.parametrize("n_ant", [4, 8])
def test_four_and_eight_copies_keep_triggers_cfo_decisions_and_psdus(n_ant):
    x = streams("one")[0]
    want = single_run("one")
    got = div_run((x,) * n_ant)
    assert np.array_equal(got["frames"]["trigger"], want["frames"]["trigger"])
    assert np.array_equal(got["frames"]["cfo_coarse"].view(np.uint32), want["frames"]["cfo_coarse"].view(np.uint32))
    same_bytes(got, want, ("idx", "psdu"))
    assert (got["used_mask"] == (1 << n_ant) - 1).all()
    assert ((got["frames"]["flags"] & capi.F_CRC_OK) != 0).all()


# ---- 4. an all-zero antenna --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zero_first", [False, True], ids=["antenna 1 zero", "antenna 0 zero"])
def test_an_all_zero_antenna_leaves_the_other_antennas_stream(zero_first):
    x = streams("one")[0]
    z = np.zeros_like(x)
    want = single_run("one")
    got = div_run((z, x) if zero_first else (x, z))
    same_bytes(got, want)
    assert (got["used_mask"] == (2 if zero_first else 1)).all()


# ---- 5. two different antennas -----------------------------------------------------------------------------------------------------

GAIN2 = (1.0, 0.5)


@functools.lru_cache(maxsize=None)
def two_base():
    return div_run(streams("two"), ant_gain=GAIN2)


@pytest.mark.parametrize("batch", [0, 20000])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_delivered_bytes_do_not_depend_on_chunk_or_batch(chunk, batch):
    got = div_run(streams("two"), chunk, batch=batch, ant_gain=GAIN2)
    same_bytes(got, two_base(), KEYS + ("used_mask", "ant_frames"))
    assert got["stats"] == two_base()["stats"]


@pytest.mark.parametrize("chunk,batch", [(0, 0), (4096, 20000)])
def test_host_input_equals_device_input(chunk, batch):
    got = div_run(streams("two"), chunk, batch=batch, ant_gain=GAIN2, on_device=True)
    same_bytes(got, two_base(), KEYS + ("used_mask", "ant_frames"))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_sc16_input_equals_fc32_input_of_the_widened_samples(on_device):
    xs = streams("two")
    scale_q = cr.full_scale(xs[0], 12.0, cr.SC16)
    scale_w = np.float32(1.0) / scale_q
    q = [cr.quantise(cr.pairs(x), scale_q, cr.SC16)[0] for x in xs]
    w = tuple(cr.to_complex(cr.widen(v, scale_w)) for v in q)
    want = div_run(w, 4096, ant_gain=GAIN2)
    got = div_run(q, 4096, ant_gain=GAIN2, on_device=on_device, fmt="sc16", scale=float(scale_w))
    assert len(want["frames"]) == 10
    same_bytes(got, want, KEYS + ("used_mask", "ant_frames"))


GAIN3 = ((1.0, 7), (0.7 * np.exp(0.8j), 8), (0.5 * np.exp(-2.0j), 9))      # (gain, noise seed) per antenna
FIRST_CAP = 1 << 16             # samples a plane holds after the first reserve (stream_reserve)


@pytest.mark.parametrize("fmt", ["fc32", "sc8"])
def test_three_planes_regrow_with_their_samples_kept(fmt):
    """The first push ends inside the first frame (samples 100 .. 2180 of the stream): its trigger stays pending and the carry
    keeps its samples in all three planes.  The second push needs more than the planes' first capacity, so the reserve moves
    three partly filled planes to a new pitch.  Delivered is, byte for byte, what one push of the same streams delivers.  The
    first push is odd, so with sc8 host input the second pass stages its chunks at the odd-fill offset of the native scratch."""
    clean, _ = sdr.clean_stream()
    clean = np.tile(clean, -(-(FIRST_CAP + 4096) // clean.size))
    xs = [sdr.antenna(clean, g, seed) for g, seed in GAIN3]
    n, first = clean.size, 1201
    kw = {}
    if fmt == "sc8":
        scale_q = cr.full_scale(xs[0], 12.0, cr.SC8)
        xs = [cr.quantise(cr.pairs(x), scale_q, cr.SC8)[0] for x in xs]
        kw = dict(fmt="sc8", scale=float(np.float32(1.0) / scale_q))
    assert first % 2 == 1 and 100 + 320 < first < 2180 and n - first + 64 > FIRST_CAP
    want = div_run(xs, **kw)
    got = div_run(xs, edges=[(0, first), (first, n)], **kw)
    assert len(want["frames"]) == 10 * (n // sdr.clean_stream()[0].size) and want["stats"]["frames_detected"] == len(want["frames"])
    same_bytes(got, want, KEYS + ("used_mask", "ant_frames"))
    assert got["stats"] == want["stats"]


def test_every_antennas_record_carries_the_joint_trigger_and_cfo():
    got = two_base()
    t, Ar, Ai = mr.detect(streams("two"), THR, MP)
    assert len(t) == len(got["frames"]) == 10
    for a in range(2):
        assert np.array_equal(got["ant_frames"][:, a]["trigger"], t)
        assert np.array_equal(got["ant_frames"][:, a]["cfo_coarse"].view(np.uint32), got["frames"]["cfo_coarse"].view(np.uint32))
    assert np.array_equal(got["frames"]["trigger"], t)
    assert (got["used_mask"] == 3).all() and ((got["frames"]["flags"] & capi.F_CRC_OK) != 0).all()
    psdus = sdr.clean_stream()[1]
    for k, p in enumerate(psdus):
        assert np.array_equal(got["psdu"][k, :len(p)], p)
    # the delivered csi / sym_stats rows: the reference antenna's, the lowest usable one whose snr_db is the combined record's
    ref = [min(a for a in range(2) if got["ant_frames"][k, a]["snr_db"] == got["frames"][k]["snr_db"]) for k in range(10)]
    assert set(ref) <= {0, 1}


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------

def test_stream_diversity_gain():
    """512 config-2 frames (294 B, QPSK 1/2) at 12 dB, flat Rayleigh independent per antenna and frame, two antennas, built on the
    device (wifirx_tx_batch, wifirx_channel_fading with doppler 0: what tests/stream_diversity_point.py's host chain builds with
    fading_ref) and pushed as two device-resident streams.  Asserted, hard and soft: lost(MRC) <= lost(SELECT), and lost(MRC) <= half
    the better antenna's own wifirx_push stream.  The batch path's count on the same rows is printed beside it, not asserted."""
    n, enc, plen = pt.N, pt.ENC, pt.PLEN
    n_sym, slot = pt.geometry()
    total = n * slot
    psdus = txgen.make_psdus(n, plen, seed=pt.PSDU_SEED)
    gen = capi.WifiRx(max_sym=n_sym, llr_bits=2, want_carrier=True)
    bufs, counts = [], {}
    try:
        d_psdu = gen.alloc(n * plen).upload(psdus)
        tx = gen.alloc(total * 8)
        ant = [gen.alloc(total * 8) for _ in pt.SEEDS]
        bufs += [d_psdu, tx] + ant
        gen.tx_batch_dev(tx.ptr, total, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=pt.LEAD, row_len=slot)
        for d, (seed, fade_seed) in zip(ant, pt.SEEDS):
            gen.channel_dev(tx.ptr, d.ptr, total, n, row_len=slot, gain=math.sqrt(10 ** (pt.SNR_DB / 10)), noise_voltage=1.0, seed=seed,
                            doppler=0.0, fade_seed=fade_seed)
        gen.sync()                              # the streams are read on other handles' streams

        def lost(frames, psdu):
            ok = np.zeros(n, bool)
            good = np.flatnonzero(((frames["flags"] & capi.F_CRC_OK) != 0) & (frames["psdu_len"] == plen))
            for k in good:
                row = int(frames["trigger"][k]) // slot
                if np.array_equal(psdu[k, :plen], psdus[row]):
                    ok[row] = True
            return int(n - ok.sum())

        def drain(rx, poll):
            fr, ps = [], []
            while True:
                r = poll(cap=1024, psdu_stride=320)
                if len(r["frames"]) == 0:
                    break
                fr.append(r["frames"])
                ps.append(r["psdu"])
            return np.concatenate(fr), np.concatenate(ps)

        for soft in (0, 1):
            for a, d in enumerate(ant):
                rx = new_handle(soft=soft, max_sym=n_sym)
                rx._check(capi.lib().wifirx_push(rx._h, d.ptr, total, 1))
                rx.flush()
                counts["ant%d" % a, soft] = lost(*drain(rx, rx.poll))
                rx.close()
            for name, mode in (("select", capi.DIV_SELECT), ("mrc", capi.DIV_MRC)):
                rx = new_handle(soft=soft, max_sym=n_sym)
                rx.push_diversity_dev([d.ptr for d in ant], total, mode)
                rx.flush_diversity(mode)
                counts[name, soft] = lost(*drain(rx, rx.poll_diversity))
                rx.close()
            # the batch path on the same rows: every row its own slot (reported, not asserted)
            ins = []
            for d in ant:
                ins.append(gen.alloc_out(n, want_csi=True))
                gen.demod_batch_dev(d.ptr, slot, n, ins[-1])
            out = gen.alloc_out(n, psdu_stride=320)
            gen.diversity_combine_dev(ins, n, out, capi.DIV_MRC)
            (gen.decode_batch_soft_dev if soft else gen.decode_batch_dev)(n, out)
            gen.sync()
            r = gen.download_out(out, n)
            okb = ((r["frames"]["flags"] & capi.F_CRC_OK) != 0) & (r["frames"]["psdu_len"] == plen) & (r["psdu"][:, :plen] == psdus).all(axis=1)
            counts["batch_mrc", soft] = int(n - okb.sum())
            for dd in ins + [out]:
                gen.free_out(dd)
        rec = {k: [counts[k, 0], counts[k, 1]] for k in ("ant0", "ant1", "select", "mrc", "batch_mrc")}
        print("lost frames of %d (hard, soft): %s" % (n, json.dumps(rec)))
        for soft in (0, 1):
            single = min(counts["ant0", soft], counts["ant1", soft])
            assert counts["mrc", soft] <= counts["select", soft], (soft, rec)
            assert 2 * counts["mrc", soft] <= single, (soft, rec)
    finally:
        for b in bufs:
            b.free()
        gen.close()


# ---- 7. all or nothing -------------------------------------------------------------------------------------------------------------

def test_a_failed_pass_consumed_nothing(monkeypatch):
    """WIFIRX_TEST_FAIL_ALLOC = k fails the handle's k-th stream allocation once (a simulated allocation failure on the host):
    that push returns ENOMEM and has consumed nothing; the same call again goes through, and the frames are those of an
    undisturbed run."""
    xs = streams("two")
    chunk = 30000
    want = div_run(xs, chunk, ant_gain=GAIN2)
    assert len(want["frames"]) == 10
    failures = 0
    for k in range(1, 22):          # 3 sample-side buffers, 8 combined rows, 6 antenna rows, and their first regrowth
        monkeypatch.setenv("WIFIRX_TEST_FAIL_ALLOC", str(k))
        rx = new_handle()
        try:
            got = []
            for a, b in cuts(len(xs[0]), chunk):
                piece = [x[a:b] for x in xs]
                before = rx.stats()
                try:
                    rx.push_diversity(piece, ant_gain=GAIN2)
                except capi.WifiRxError as e:
                    assert e.code == capi.ENOMEM, str(e)
                    failures += 1
                    assert rx.stats() == before and rx.queued() == 0
                    rx.push_diversity(piece, ant_gain=GAIN2)
                got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
            try:
                rx.flush_diversity(ant_gain=GAIN2)
            except capi.WifiRxError as e:
                assert e.code == capi.ENOMEM, str(e)
                failures += 1
                rx.flush_diversity(ant_gain=GAIN2)
            got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
            same_bytes(collect(rx, got, KEYS + ("used_mask", "ant_frames")), want, KEYS + ("used_mask", "ant_frames"))
        finally:
            rx.close()
    assert failures >= 12


def test_a_failed_pass_of_host_integers_consumed_nothing(monkeypatch):
    """test_a_failed_pass_consumed_nothing with sc16 host input: the native scratch is one more allocation in the numbered
    sequence (behind the three sample-side buffers), so one k more is covered and one failure more is the least."""
    xs = streams("two")
    scale_q = cr.full_scale(xs[0], 12.0, cr.SC16)
    q = [cr.quantise(cr.pairs(x), scale_q, cr.SC16)[0] for x in xs]
    kw = dict(ant_gain=GAIN2, fmt="sc16", scale=float(np.float32(1.0) / scale_q))
    chunk = 30000
    want = div_run(q, chunk, **kw)
    assert len(want["frames"]) == 10
    failures = 0
    for k in range(1, 23):
        monkeypatch.setenv("WIFIRX_TEST_FAIL_ALLOC", str(k))
        rx = new_handle()
        try:
            got = []
            for a, b in cuts(len(q[0]), chunk):
                piece = [x[a:b] for x in q]
                before = rx.stats()
                try:
                    rx.push_diversity(piece, **kw)
                except capi.WifiRxError as e:
                    assert e.code == capi.ENOMEM, str(e)
                    failures += 1
                    assert rx.stats() == before and rx.queued() == 0
                    rx.push_diversity(piece, **kw)
                got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
            try:
                rx.flush_diversity(ant_gain=GAIN2)
            except capi.WifiRxError as e:
                assert e.code == capi.ENOMEM, str(e)
                failures += 1
                rx.flush_diversity(ant_gain=GAIN2)
            got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
            same_bytes(collect(rx, got, KEYS + ("used_mask", "ant_frames")), want, KEYS + ("used_mask", "ant_frames"))
        finally:
            rx.close()
    assert failures >= 13


@pytest.mark.parametrize("when", [1, -1], ids=["before the move", "after the move began"])
def test_a_failed_carry_is_never_a_failed_push(monkeypatch, when):
    """WIFIRX_TEST_FAIL_CARRY (a simulated failure on the host, behind the commit of a pass), as for the single stream: struck
    before the planes were touched the stream goes on unharmed; after, every later push is WIFIRX_EDEAD and the frames up to
    there were delivered."""
    xs = streams("two")
    want = two_base()
    monkeypatch.setenv("WIFIRX_TEST_FAIL_CARRY", str(when))
    rx = new_handle()
    try:
        got, dead = [], False
        for a, b in cuts(len(xs[0]), 8192):
            try:
                rx.push_diversity([x[a:b] for x in xs], ant_gain=GAIN2)
            except capi.WifiRxError as e:
                assert e.code == capi.EDEAD and when < 0 and "destroy the handle" in str(e)
                dead = True
                break
            got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
        if when > 0:
            rx.flush_diversity(ant_gain=GAIN2)
            got.append(rx.poll_diversity(cap=64, want_idx=True, want_csi=True, want_stats=True))
            same_bytes(collect(rx, got, KEYS + ("used_mask", "ant_frames")), want, KEYS + ("used_mask", "ant_frames"))
        else:
            assert dead
            with pytest.raises(capi.WifiRxError) as ei:
                rx.flush_diversity(ant_gain=GAIN2)
            assert ei.value.code == capi.EDEAD
            n = sum(len(g["frames"]) for g in got)
            if n:
                fr = np.concatenate([g["frames"] for g in got])
                assert np.array_equal(fr, want["frames"][:n])
    finally:
        rx.close()


# ---- 8. refused arguments ----------------------------------------------------------------------------------------------------------

def test_every_refused_argument_returns_its_code_and_queues_nothing():
    lib, E = capi.lib(), capi.EINVAL
    x = np.ascontiguousarray(streams("one")[0][:4096])
    rx = capi.WifiRx(max_sym=64)
    other = capi.WifiRx(max_sym=64)
    d = rx.alloc(x.nbytes + 64).upload(x)
    d_m, d_A = rx.alloc(8 * 80), rx.alloc(8 * 4200)
    try:
        ptrs2 = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
        g_ok = (C.c_float * 2)(1.0, 0.5)

        def push(n_ant=2, mode=0, gain=None, fmt=0, scale=1.0, on_dev=0, iq=ptrs2, n=x.size, cfg=True, h=rx):
            c = capi.DivStream(n_ant, mode, gain, fmt, scale, on_dev)
            return lib.wifirx_push_diversity(h._h if h else None, C.byref(c) if cfg else None, iq, n)

        null_ant = (C.c_void_p * 2)(x.ctypes.data, None)
        odd_dev = (C.c_void_p * 2)(d.ptr, d.ptr + 4)
        odd_sc16 = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data + 2)
        bad = {
            "null handle": push(h=None), "null cfg": push(cfg=False), "null iq": push(iq=None), "null iq[a]": push(iq=null_ant),
            "n_ant 0": push(n_ant=0), "n_ant 9": push(n_ant=9), "mode": push(mode=2), "fmt": push(fmt=3), "fmt -1": push(fmt=-1),
            "gain < 0": push(gain=(C.c_float * 2)(1.0, -0.5)), "gain nan": push(gain=(C.c_float * 2)(float("nan"), 1.0)),
            "gain inf": push(gain=(C.c_float * 2)(1.0, float("inf"))), "scale 0": push(fmt=1, scale=0.0),
            "misaligned device": push(on_dev=1, iq=odd_dev), "misaligned sc16": push(fmt=1, scale=2.0 ** -15, iq=odd_sc16),
        }
        assert all(v == E for v in bad.values()), bad
        assert rx.queued() == 0 and rx.stats()["samples_in"] == 0
        # the first good call fixes n_ant; another n_ant is refused from then on, and so is the single stream's entry
        assert push(gain=g_ok) == capi.OK
        assert push(n_ant=1) == E and push(n_ant=3, iq=(C.c_void_p * 3)(*[x.ctypes.data] * 3)) == E
        st = rx.stats()
        assert st["samples_in"] == x.size
        assert lib.wifirx_push(rx._h, x.ctypes.data, x.size, 0) == E and lib.wifirx_push(rx._h, None, 0, 0) == E
        assert lib.wifirx_push_iq(rx._h, x.ctypes.data, x.size // 2, 1, 2.0 ** -15, 0) == E
        assert rx.stats() == st
        # ... and the reverse
        other.push(x)
        st = other.stats()
        assert push(h=other) == E and push(h=other, n=0) == E and other.stats() == st
        # wifirx_detect_multi
        iq1 = (C.c_void_p * 1)(d.ptr)

        def detect(n_ant=1, iq=iq1, n=4096, thr=0.56, m=d_m.ptr, A=d_A.ptr, P=None, h=rx):
            return lib.wifirx_detect_multi(h._h if h else None, n_ant, iq, n, thr, m, A, P)

        bad = {
            "null handle": detect(h=None), "null iq": detect(iq=None), "null iq[a]": detect(iq=(C.c_void_p * 1)(None)),
            "n_ant 0": detect(n_ant=0), "n_ant 9": detect(n_ant=9), "thr < 0": detect(thr=-0.1), "thr nan": detect(thr=float("nan")),
            "null masks": detect(m=None), "null A": detect(A=None), "iq misaligned": detect(iq=(C.c_void_p * 1)(d.ptr + 4)),
            "masks misaligned": detect(m=d_m.ptr + 4), "A misaligned": detect(A=d_A.ptr + 4), "P misaligned": detect(P=d_A.ptr + 2),
        }
        assert all(v == E for v in bad.values()), bad
        assert detect() == capi.OK and detect(n=0, m=None, A=None) == capi.OK
        rx.sync()
        n_out = C.c_uint32(9)
        assert lib.wifirx_poll_diversity(rx._h, None, None, None, 4, C.byref(n_out)) == E
    finally:
        d.free(); d_m.free(); d_A.free()
        rx.close()
        other.close()


# ---- 9. the block ------------------------------------------------------------------------------------------------------------------

def test_block_with_two_antennas_publishes_the_capi_pdus():
    from wifirx import block, grshim
    xs = streams("two")
    want = two_base()                       # (ant_gain = GAIN2)
    got = []
    blk = block.wifi_phy_rx(bandwidth=20e6, antennas=2, ant_gain=GAIN2, batch_samples=20000)
    try:
        assert blk.in_sig == [np.complex64, np.complex64]
        grshim.msg_connect(blk, "mac_out", grshim.sink_block(got.append), "in")
        n = len(xs[0])
        pos = 0
        while pos < n:
            took = blk.work([xs[0][pos:pos + 8192], xs[1][pos:pos + 8192 + 100]], [])       # the common length is consumed
            assert took == min(8192, n - pos)
            pos += took
        blk.stop()
    finally:
        blk.close()
    ok = np.flatnonzero((want["frames"]["flags"] & capi.F_CRC_OK) != 0)
    assert len(got) == len(ok) == 10
    for (meta, blob), k in zip(got, ok):
        L = int(want["frames"]["psdu_len"][k])
        assert np.array_equal(blob, want["psdu"][k, :L - 4])
        assert meta["antennas_used"] == int(want["used_mask"][k]) == 3
        assert meta["frame_bytes"] == L and meta["encoding"] == int(want["frames"]["encoding"][k])
