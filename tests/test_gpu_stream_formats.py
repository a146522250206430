"""wifirx_push_iq: a stream that arrives as sc16 / sc8 gives, byte for byte, what wifirx_push gives from the rule-20 widened
samples -- and what the oracle's stream driver gives from them.  The stream is tests/stream_formats_case.py's; every case
runs once."""
import functools

import numpy as np
import pytest

import convert_ref as cr
import stream_formats_case as case
from wifirx import capi

pytestmark = pytest.mark.gpu

CHUNKS = (1, 7, 4096)                       # then the rest
KEYS = ("frames", "psdu", "idx", "carrier", "csi", "sym_stats")
FMT_NAME = {cr.SC16: "sc16", cr.SC8: "sc8"}


def cuts(n):
    pos, out = 0, []
    for c in CHUNKS + (n,):
        out.append((pos, min(pos + c, n)))
        pos = out[-1][1]
    return [(a, b) for a, b in out if b > a]


def poll_into(rx, got):
    got.append(rx.poll(cap=64, want_idx=True, want_csi=True, want_stats=True))


def collect(rx, got):
    out = {k: np.concatenate([g[k] for g in got]) for k in KEYS}
    out["stats"] = rx.stats()
    return out


def new_handle(batch=0, soft=0):
    rx = capi.WifiRx(max_sym=511, want_carrier=True)
    rx.set_param(capi.P_STREAM_BATCH, batch)
    rx.set_param(capi.P_STREAM_SOFT, soft)
    return rx


@functools.lru_cache(maxsize=None)
def float_result(fmt, soft=0):
    """the second handle: the widened float32 samples through wifirx_push, in the same chunks (computed once per format)"""
    w = case.stream(fmt)[4]
    rx = new_handle(soft=soft)
    try:
        got = []
        for a, b in cuts(w.size):
            rx.push(w[a:b])
            poll_into(rx, got)
        rx.flush()
        poll_into(rx, got)
        return collect(rx, got)
    finally:
        rx.close()


def assert_same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert got["stats"] == want["stats"]


def assert_oracle(got, fmt, soft=False):
    o, opsdu = case.oracle_result(fmt, soft)
    psdus = case.stream(fmt)[1]
    fr = got["frames"]
    assert np.array_equal(fr, o["frames"]), (fr, o["frames"])
    assert len(fr) == len(psdus) and ((fr["flags"] & capi.F_CRC_OK) != 0).all()
    for k in range(len(fr)):
        n, L = int(fr["n_sym_out"][k]), int(fr["psdu_len"][k])
        assert np.array_equal(got["idx"][k, :n], o["idx"][k, :n])
        assert np.array_equal(got["carrier"][k, :n], o["eq"][k, :n])
        assert np.array_equal(got["psdu"][k, :L], opsdu[k, :L]) and np.array_equal(got["psdu"][k, :L], psdus[k])
    assert got["stats"]["samples_in"] == case.stream(fmt)[0].size


def run_push_iq(fmt, batch, on_device, soft=0):
    _, _, q, _, _, scale_w = case.stream(fmt)
    rx = new_handle(batch, soft)
    d_q = None
    try:
        got = []
        if on_device:
            d_q = rx.alloc(q.nbytes).upload(q)
        for a, b in cuts(len(q)):
            if on_device:
                rx.push_iq_dev(d_q.ptr + a * q.itemsize * 2, b - a, fmt, scale_w)
            else:
                rx.push_iq(q[a:b], scale=scale_w)
            assert rx.push_consumed() == b - a
            poll_into(rx, got)
        rx.flush()
        poll_into(rx, got)
        return collect(rx, got)
    finally:
        if d_q is not None:
            d_q.free()
        rx.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("batch", [0, 8192])
@pytest.mark.parametrize("fmt", [cr.SC16, cr.SC8], ids=["sc16", "sc8"])
def test_push_iq_equals_push_of_the_widened_samples(fmt, batch, on_device):
    got = run_push_iq(fmt, batch, on_device)
    assert_same(got, float_result(fmt))
    assert_oracle(got, fmt)


def test_push_iq_soft_decision_stream():
    got = run_push_iq(cr.SC16, 8192, False, soft=1)
    assert_same(got, float_result(cr.SC16, soft=1))
    assert_oracle(got, cr.SC16, soft=True)


@pytest.mark.parametrize("batch", [0, 8192])
def test_formats_alternate_within_a_stream(batch):
    """the first half as sc16 through push_iq, the second as float32 through wifirx_push -- cut at an odd sample in the middle
    of a frame, with samples of the first format still staged when the second arrives"""
    _, _, q, _, w, scale_w = case.stream(cr.SC16)
    half = len(q) // 2 + 1
    rx = new_handle(batch)
    try:
        got = []
        for a, b in cuts(half):
            rx.push_iq(q[a:b], scale=scale_w)
            poll_into(rx, got)
        rx.push(w[half:half + 3])
        rx.push_iq(q[half + 3:half + 8], scale=scale_w)
        rx.push(w[half + 8:])
        assert rx.push_consumed() == w.size - half - 8
        poll_into(rx, got)
        rx.flush()
        poll_into(rx, got)
        res = collect(rx, got)
    finally:
        rx.close()
    assert_same(res, float_result(cr.SC16))


@pytest.mark.parametrize("batch", [0, 8192])
def test_fc32_through_push_iq_is_push(batch):
    w = case.stream(cr.SC16)[4]
    rx = new_handle(batch)
    try:
        got = []
        for a, b in cuts(w.size):
            rx.push_iq(w[a:b], fmt="fc32", scale=float("nan"))      # the scale is not looked at
            assert rx.push_consumed() == b - a
            poll_into(rx, got)
        rx.flush()
        poll_into(rx, got)
        res = collect(rx, got)
    finally:
        rx.close()
    assert_same(res, float_result(cr.SC16))


@pytest.mark.parametrize("batch", [0, 8192])
def test_bad_format_or_scale_is_refused_and_the_stream_goes_on(batch):
    _, _, q, _, _, scale_w = case.stream(cr.SC8)
    lib = capi.lib()
    rx = new_handle(batch)
    try:
        got = []
        cut = cuts(len(q))
        for i, (a, b) in enumerate(cut):
            if i == 2:          # in mid-stream, with samples staged or carried
                part = np.ascontiguousarray(q[a:b])
                ptr = part.ctypes.data
                for fmt, scale, p in ((3, 1.0, ptr), (-1, 1.0, ptr), (cr.SC8, 0.0, ptr), (cr.SC8, -1.0, ptr), (cr.SC8, float("nan"), ptr),
                                      (cr.SC16, float("inf"), ptr), (cr.SC8, 1.0, ptr + 1), (cr.SC16, 1.0, ptr + 2), (cr.SC8, 1.0, None)):
                    assert lib.wifirx_push_iq(rx._h, p, b - a, fmt, scale, 0) == capi.EINVAL, (fmt, scale)
                    assert rx.push_consumed() == 0
            rx.push_iq(q[a:b], scale=scale_w)
            poll_into(rx, got)
        rx.flush()
        poll_into(rx, got)
        res = collect(rx, got)
    finally:
        rx.close()
    assert_same(res, float_result(cr.SC8))


def test_block_with_sc16_items_publishes_the_pdus_of_the_fc32_block():
    from wifirx import block, grshim
    _, psdus, q, _, w, scale_w = case.stream(cr.SC16)

    def run(samples, **kw):
        pdus = []
        blk = block.wifi_phy_rx(bandwidth=20e6, publish_carrier=False, batch_samples=8192, **kw)
        try:
            grshim.msg_connect(blk, "mac_out", grshim.sink_block(pdus.append), "in")
            assert grshim.run_stream(blk, samples, chunk=4096) == len(samples)
            return pdus, blk.stats()
        finally:
            blk.close()

    got, st_i = run(q, sample_format="sc16", sample_scale=scale_w)
    want, st_f = run(w)
    assert len(got) == len(want) == len(psdus) and st_i == st_f
    for (gm, gb), (wm, wb), p in zip(got, want, psdus):
        assert gm == wm and np.array_equal(gb, wb) and np.array_equal(gb, p[:-4])
