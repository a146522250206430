"""bf16 LLR rows (WIFIRX_P_LLR_FORMAT = WIFIRX_LLR_BF16, NUMERICS.md rule 15) on the MI355X: the parameter's values; the
bf16 bits equal the round-to-nearest-even conversion of the float32 LLRs -- of a twin handle in the default format on the
same input and of the oracle -- at every rate, equaliser, llr_csi and llr_bits, with every other output byte-identical;
the store paths the usual loops do not take (mixed-rate waves, a 2-byte aligned `llr`, demod_batch_v, host outputs,
wifirx_time_demod); channel-state-weighted LLRs beyond float16's range; a fenced buffer of exactly the bf16 size; and
wifirx_decode_batch_soft on bf16 rows against tests/soft_viterbi_ref.py."""
import ctypes as C

import numpy as np
import pytest

import soft_viterbi_ref as ref
from helpers import make_slots
from llr_bf16_ref import bf16_rne, bf16_to_f32, same_bf16
from wifirx import txgen

pytestmark = pytest.mark.gpu

NBPSC = (1, 1, 2, 2, 4, 4, 6, 6)


@pytest.fixture(scope="module")
def capi():
    from wifirx import capi
    return capi


def run_dev(capi, rx, iq, slot_len, n, **kw):
    """demod into device buffers of the handle's format, then download every output"""
    dev = rx.alloc_out(n, **kw)
    d_iq = rx.alloc(iq.nbytes).upload(iq)
    try:
        rx.demod_batch_dev(d_iq.ptr, slot_len, n, dev)
        rx.sync()
        return rx.download_out(dev, n)
    finally:
        d_iq.free()
        rx.free_out(dev)


def twins(capi, **kw):
    return capi.WifiRx(device=0, **kw), capi.WifiRx(device=0, llr_format="bf16", **kw)


def assert_rest_equal(a, b):
    for k in ("frames", "idx", "hbits", "carrier", "csi", "sym_stats"):
        if a.get(k) is not None or b.get(k) is not None:
            assert a[k].tobytes() == b[k].tobytes(), k


def test_parameter_values(capi):
    rx = capi.WifiRx(max_sym=8, llr_bits=2, device=0)
    try:
        lib = capi.lib()
        for v in (0.0, 1.0, 0.0):
            assert lib.wifirx_set_param(rx._h, capi.P_LLR_FORMAT, C.c_double(v)) == capi.OK
        for v in (2.0, -1.0, 0.5):
            assert lib.wifirx_set_param(rx._h, capi.P_LLR_FORMAT, C.c_double(v)) == capi.EINVAL
        rx.set_llr_format("bf16")
        assert rx.llr_format == capi.LLR_BF16
        with pytest.raises(capi.WifiRxError):
            rx.set_param(capi.P_LLR_FORMAT, 2)
        assert rx.llr_format == capi.LLR_BF16
        rx.set_param(capi.P_LLR_FORMAT, 0)
        assert rx.llr_format == capi.LLR_F32
    finally:
        rx.close()


@pytest.mark.parametrize("eq", [0, 1, 2, 3])
@pytest.mark.parametrize("csi", [0, 1])
def test_parity_matrix(capi, orc, eq, csi):
    """8 encodings x llr_bits n_bpsc..6: bf16 bits = bf16(float32 twin) = bf16(oracle); every other output identical"""
    for enc in range(8):
        n = 16
        iq, slot_len, tx = make_slots(n, enc, psdu_len=40 + 9 * enc, snr_db=18.0, seed=300 + 10 * enc + eq + 5 * csi)
        for lb in (1, 2, 4, 6):
            if lb < NBPSC[enc]:
                continue
            kw = dict(max_sym=tx.n_sym, llr_bits=lb, chan_est=eq)
            a, b = twins(capi, **kw)
            try:
                a.set_param(capi.P_LLR_CSI, csi)
                b.set_param(capi.P_LLR_CSI, csi)
                ra = run_dev(capi, a, iq, slot_len, n, want_hbits=True)
                rb = run_dev(capi, b, iq, slot_len, n, want_hbits=True)
            finally:
                a.close()
                b.close()
            assert rb["llr"].dtype == np.uint16 and rb["llr"].shape == ra["llr"].shape
            assert same_bf16(rb["llr"], bf16_rne(ra["llr"])), (enc, lb)
            assert_rest_equal(ra, rb)
            o = orc.demod_batch(iq, slot_len, orc.make_params(max_sym=tx.n_sym, llr_bits=lb, chan_est=eq, llr_csi=csi))
            assert same_bf16(rb["llr"], bf16_rne(o["llr"])), (enc, lb)
            assert ((rb["frames"]["flags"] & capi.F_LLR) != 0).sum() > n // 2


@pytest.mark.parametrize("eq", [0, 1])
def test_every_output_with_carrier_and_stats(capi, eq):
    """the any-set (XK) loops: equalised points, channel state, moments and planes beside bf16 LLRs"""
    for enc in (0, 2, 4, 7):
        n = 12
        iq, slot_len, tx = make_slots(n, enc, psdu_len=60, snr_db=20.0, seed=500 + enc)
        a, b = twins(capi, max_sym=tx.n_sym, llr_bits=6, chan_est=eq, want_carrier=True)
        try:
            for csi in (0, 1):
                a.set_param(capi.P_LLR_CSI, csi)
                b.set_param(capi.P_LLR_CSI, csi)
                kw = dict(want_csi=True, want_stats=True, want_hbits=True)
                ra, rb = run_dev(capi, a, iq, slot_len, n, **kw), run_dev(capi, b, iq, slot_len, n, **kw)
                assert same_bf16(rb["llr"], bf16_rne(ra["llr"])), (enc, csi)
                assert_rest_equal(ra, rb)
        finally:
            a.close()
            b.close()


def mixed_slots(n, snr_db, seed, lens=(40, 150, 300)):
    """frame k of rate k % 8 and length lens[(k // 8) % len(lens)]: waves of mixed rates and lengths"""
    rng = np.random.default_rng(seed)
    encs = np.arange(n) % 8
    ln = np.array(lens)[(np.arange(n) // 8) % len(lens)]
    sig = [txgen.encode_psdus(txgen.make_psdus(1, int(l_), seed=seed * 1000 + k), int(e)).samples[0]
           for k, (e, l_) in enumerate(zip(encs, ln))]
    n_max = max(s.size for s in sig)
    frames = np.zeros((n, n_max), np.complex64)
    for k, s in enumerate(sig):
        frames[k, :s.size] = s
    slot_len = ((160 + n_max + 320 + 63) // 64) * 64
    x = txgen.impair(frames, snr_db, cfo=rng.uniform(-4e-4, 4e-4, n), lead=160, total=slot_len, seed=seed + 17)
    return x.reshape(-1), slot_len, txgen.n_sym_for(max(lens), 0)


@pytest.mark.parametrize("csi", [0, 1])
def test_mixed_rate_waves(capi, csi):
    n = 72
    iq, slot_len, ms = mixed_slots(n, 14.0, seed=61 + csi)
    a, b = twins(capi, max_sym=ms, llr_bits=6)
    try:
        a.set_param(capi.P_LLR_CSI, csi)
        b.set_param(capi.P_LLR_CSI, csi)
        ra, rb = run_dev(capi, a, iq, slot_len, n), run_dev(capi, b, iq, slot_len, n)
    finally:
        a.close()
        b.close()
    assert same_bf16(rb["llr"], bf16_rne(ra["llr"]))
    assert_rest_equal(ra, rb)


def test_two_byte_aligned_llr(capi):
    """an `llr` pointer 2 bytes past a 16-byte boundary takes the per-value stores"""
    n, enc = 16, 3
    iq, slot_len, tx = make_slots(n, enc, psdu_len=100, snr_db=18.0, seed=71)
    a, b = twins(capi, max_sym=tx.n_sym, llr_bits=2)
    try:
        ra = run_dev(capi, a, iq, slot_len, n)
        nv = n * tx.n_sym * 48 * 2
        buf = b.alloc(2 * nv + 32).upload(np.full(2 * nv + 32, 0xA5, np.uint8))
        fr = b.alloc(n * 32)
        idx = b.alloc(n * tx.n_sym * 48)
        d_iq = b.alloc(iq.nbytes).upload(iq)
        try:
            out = capi.Out(fr.ptr, idx.ptr, buf.ptr + 2, None, None, 0, 1, None, None, None)
            b._check(capi.lib().wifirx_demod_batch(b._h, d_iq.ptr, 1, slot_len, n, C.byref(out)))
            b.sync()
            raw = buf.download(np.uint16, nv + 16)
            frames = fr.download(capi.FRAME_DTYPE, n)
            idx_b = idx.download(np.uint8, n * tx.n_sym * 48).reshape(n, tx.n_sym, 48)
        finally:
            for d in (buf, fr, idx, d_iq):
                d.free()
    finally:
        a.close()
        b.close()
    assert raw[0] == 0xA5A5 and (raw[1 + nv:] == 0xA5A5).all()
    got = raw[1:1 + nv].reshape(n, -1)
    written = np.zeros_like(got, dtype=bool)
    for k in range(n):
        if frames["flags"][k] & capi.F_LLR:
            written[k, :frames["n_sym_out"][k] * 48 * frames["n_bpsc"][k]] = True
    assert written.sum() > 0
    assert same_bf16(got[written], bf16_rne(ra["llr"])[written])
    assert np.array_equal(frames, ra["frames"]) and np.array_equal(idx_b, ra["idx"])


def test_demod_batch_v(capi):
    iq, slot_len, ms = mixed_slots(24, 16.0, seed=81)
    per = iq.reshape(24, slot_len)
    cut = [slot_len - 64 * (k % 3) for k in range(24)]
    x = np.concatenate([per[k, :cut[k]] for k in range(24)])
    off = np.concatenate([[0], np.cumsum(cut)]).astype(np.uint64)
    a, b = twins(capi, max_sym=ms, llr_bits=6)
    try:
        ra, rb = a.demod_batch_var(x, off), b.demod_batch_var(x, off)
    finally:
        a.close()
        b.close()
    assert rb["llr"].dtype == np.uint16
    assert same_bf16(rb["llr"], bf16_rne(ra["llr"]))
    assert np.array_equal(ra["frames"], rb["frames"]) and np.array_equal(ra["idx"], rb["idx"])


def test_host_outputs_and_time_demod(capi):
    n, enc = 40, 5
    iq, slot_len, tx = make_slots(n, enc, psdu_len=120, snr_db=22.0, seed=91)
    a, b = twins(capi, max_sym=tx.n_sym, llr_bits=4, want_carrier=True)
    try:
        ha = a.demod_batch(iq, slot_len, want_csi=True, want_stats=True, want_hbits=True)
        hb = b.demod_batch(iq, slot_len, want_csi=True, want_stats=True, want_hbits=True)
        assert hb["llr"].dtype == np.uint16
        assert same_bf16(hb["llr"], bf16_rne(ha["llr"]))
        assert_rest_equal(ha, hb)
        # wifirx_time_demod leaves the rows demod_batch writes
        dev = b.alloc_out(n)
        d_iq = b.alloc(iq.nbytes).upload(iq)
        try:
            ms = b.time_demod(d_iq.ptr, slot_len, n, dev, iters=2)
            assert ms > 0
            rt = b.download_out(dev, n)
        finally:
            d_iq.free()
            b.free_out(dev)
        assert np.array_equal(rt["llr"], hb["llr"]) and np.array_equal(rt["frames"], hb["frames"])
    finally:
        a.close()
        b.close()


def test_large_weighted_llrs(capi):
    """input x 1e4 with llr_csi 1: |H|^2 ~ 1e8 -- beyond float16, inside bf16's range"""
    n, enc = 16, 6
    iq, slot_len, tx = make_slots(n, enc, psdu_len=80, snr_db=25.0, seed=101)
    iq = (iq * np.float32(1e4)).astype(np.complex64)
    a, b = twins(capi, max_sym=tx.n_sym, llr_bits=6)
    try:
        for rx in (a, b):
            rx.set_param(capi.P_LLR_CSI, 1)
        ra, rb = run_dev(capi, a, iq, slot_len, n), run_dev(capi, b, iq, slot_len, n)
    finally:
        a.close()
        b.close()
    assert np.nanmax(np.abs(ra["llr"])) > 65504.0
    assert same_bf16(rb["llr"], bf16_rne(ra["llr"]))
    assert np.isfinite(bf16_to_f32(rb["llr"])).all()


@pytest.mark.parametrize("enc", [0, 3, 4, 7])
def test_fenced_buffer(capi, enc):
    """the LLR buffer is exactly n_slots*max_sym*48*llr_bits*2 bytes between 1 MB fences of 0xA5: the fences stay, and
    nothing is written behind a frame's n_sym_out rows"""
    n, lb, fence = 20, 6, 1 << 20
    iq, slot_len, tx = make_slots(n, enc, psdu_len=70, snr_db=20.0, seed=111 + enc)
    ms = tx.n_sym + 2                                   # rows the frames do not fill
    nv = n * ms * 48 * lb
    rx = capi.WifiRx(max_sym=ms, llr_bits=lb, device=0, llr_format="bf16")
    try:
        buf = rx.alloc(2 * fence + 2 * nv).upload(np.full(2 * fence + 2 * nv, 0xA5, np.uint8))
        fr = rx.alloc(n * 32)
        idx = rx.alloc(n * ms * 48)
        d_iq = rx.alloc(iq.nbytes).upload(iq)
        try:
            out = capi.Out(fr.ptr, idx.ptr, buf.ptr + fence, None, None, 0, 1, None, None, None)
            rx._check(capi.lib().wifirx_demod_batch(rx._h, d_iq.ptr, 1, slot_len, n, C.byref(out)))
            rx.sync()
            raw = buf.download(np.uint8, 2 * fence + 2 * nv)
            frames = fr.download(capi.FRAME_DTYPE, n)
        finally:
            for d in (buf, fr, idx, d_iq):
                d.free()
    finally:
        rx.close()
    assert (raw[:fence] == 0xA5).all() and (raw[fence + 2 * nv:] == 0xA5).all()
    rows = raw[fence:fence + 2 * nv].view(np.uint16).reshape(n, -1)
    assert ((frames["flags"] & capi.F_LLR) != 0).sum() == n
    for k in range(n):
        end = frames["n_sym_out"][k] * 48 * frames["n_bpsc"][k]
        assert end > 0 and (rows[k, end:] == 0xA5A5).all(), k


def soft_on_bf16(capi, iq, slot_len, n, ms, csi=0):
    rx = capi.WifiRx(max_sym=ms, llr_bits=6, device=0, llr_format="bf16")
    try:
        rx.set_param(capi.P_LLR_CSI, csi)
        dev = rx.alloc_out(n, psdu_stride=512)
        d_iq = rx.alloc(iq.nbytes).upload(iq)
        try:
            rx.demod_batch_dev(d_iq.ptr, slot_len, n, dev)
            rx.sync()
            r0 = rx.download_out(dev, n)
            rx.decode_batch_soft_dev(n, dev)
            rx.sync()
            return r0, rx.download_out(dev, n)
        finally:
            d_iq.free()
            rx.free_out(dev)
    finally:
        rx.close()


@pytest.mark.parametrize("n,snr,csi", [(40, 12.0, 0), (200, 12.0, 1), (136, 16.0, 0)])
def test_soft_decode_on_bf16_rows(capi, n, snr, csi):
    iq, slot_len, ms = mixed_slots(n, snr, seed=121 + n + csi)
    r0, r = soft_on_bf16(capi, iq, slot_len, n, ms, csi)
    assert r["llr"].dtype == np.uint16
    fr, psdu = ref.decode_batch(r0["frames"], bf16_to_f32(r0["llr"]), ms, psdu_stride=512)
    assert np.array_equal(r["frames"], fr)
    assert np.array_equal(r["psdu"], psdu)
    dec = (fr["flags"] & ref.F_DECODED) != 0
    assert dec.sum() > n // 3 and ((fr["flags"] & ref.F_CRC_OK) != 0).sum() > 0


def test_pm1_bf16_llrs_give_the_hard_decoder(capi):
    n = 200
    iq, slot_len, ms = mixed_slots(n, 10.0, seed=131)
    rx = capi.WifiRx(max_sym=ms, llr_bits=6, device=0, llr_format="bf16")
    try:
        dev = rx.alloc_out(n, psdu_stride=512, want_hbits=True)
        d_iq = rx.alloc(iq.nbytes).upload(iq)
        try:
            rx.demod_batch_dev(d_iq.ptr, slot_len, n, dev)
            rx.sync()
            r0 = rx.download_out(dev, n)
            dev["llr"].upload(bf16_rne(ref.pm1_llrs(r0["frames"], r0["idx"], ms, 6)))
            rx.decode_batch_soft_dev(n, dev)
            rx.sync()
            rs = rx.download_out(dev, n)
            dev["frames"].upload(r0["frames"])
            dev["psdu"].upload(np.zeros(n * 512, np.uint8))
            rx.decode_batch_dev(n, dev)
            rx.sync()
            rh = rx.download_out(dev, n)
        finally:
            d_iq.free()
            rx.free_out(dev)
    finally:
        rx.close()
    assert ((rh["frames"]["flags"] & ref.F_CRC_OK) != 0).sum() > 0
    assert np.array_equal(rs["frames"], rh["frames"]) and np.array_equal(rs["psdu"], rh["psdu"])


def test_non_finite_bf16_llrs_count_as_zero(capi):
    n = 64
    iq, slot_len, tx = make_slots(n, 3, psdu_len=120, snr_db=12.0, seed=141)
    rx = capi.WifiRx(max_sym=tx.n_sym, llr_bits=6, device=0, llr_format="bf16")
    try:
        dev = rx.alloc_out(n, psdu_stride=256)
        d_iq = rx.alloc(iq.nbytes).upload(iq)
        try:
            rx.demod_batch_dev(d_iq.ptr, slot_len, n, dev)
            rx.sync()
            r0 = rx.download_out(dev, n)
            rng = np.random.default_rng(2)
            hit = rng.random(r0["llr"].shape) < 0.02
            bad = rng.choice(np.array([0x7FC0, 0x7F80, 0xFF80, 0xFFC1], np.uint16), size=r0["llr"].shape)
            res = []
            for rows in (np.where(hit, bad, r0["llr"]), np.where(hit, np.uint16(0), r0["llr"])):
                dev["frames"].upload(r0["frames"])
                dev["psdu"].upload(np.zeros(n * 256, np.uint8))
                dev["llr"].upload(rows.astype(np.uint16))
                rx.decode_batch_soft_dev(n, dev)
                rx.sync()
                res.append(rx.download_out(dev, n))
        finally:
            d_iq.free()
            rx.free_out(dev)
    finally:
        rx.close()
    assert ((res[0]["frames"]["flags"] & ref.F_DECODED) != 0).sum() > 0
    assert np.array_equal(res[0]["frames"], res[1]["frames"]) and np.array_equal(res[0]["psdu"], res[1]["psdu"])


def test_python_binding_bf16(capi):
    n, enc = 32, 2
    iq, slot_len, tx = make_slots(n, enc, psdu_len=200, snr_db=15.0, seed=151)
    a = capi.WifiRx(max_sym=tx.n_sym, llr_bits=2, device=0)
    b = capi.WifiRx(max_sym=tx.n_sym, llr_bits=2, device=0, llr_format="bf16")
    try:
        ra = a.demod_batch(iq, slot_len, decode=True, soft=True, psdu_stride=256)
        rb = b.demod_batch(iq, slot_len, decode=True, soft=True, psdu_stride=256)
        assert rb["llr"].dtype == np.uint16 and ra["llr"].dtype == np.float32
        assert same_bf16(rb["llr"], bf16_rne(ra["llr"]))
        assert np.array_equal(capi.bf16_to_f32(rb["llr"]), bf16_to_f32(rb["llr"]))
        ok = (rb["frames"]["flags"] & capi.F_CRC_OK) != 0
        assert ok.sum() > n // 2 and np.array_equal(rb["psdu"][ok, :200], tx.psdu[ok])
        b.set_llr_format("f32")
        rc = b.demod_batch(iq, slot_len)
        assert rc["llr"].dtype == np.float32 and np.array_equal(rc["llr"], ra["llr"])
    finally:
        a.close()
        b.close()
