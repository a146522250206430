"""The detect phase on the device, on the host-built inputs of tests/detect_rows.py: batch mode (detect_quad), stream mode
(stream_detect_kernel + the host's mask state machine, any chunking, staged or not, across the carry) and the sensitivity
switched between pushes -- against the restatement of tests/detect_ref.py bit for bit and against the oracle's whole
records; the refusal of a sensitivity the squared comparison cannot honour."""
import numpy as np
import pytest

import detect_ref as ref
import detect_rows as rows
from helpers import Fenced

pytestmark = pytest.mark.gpu
F16 = np.float32(16)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr


@pytest.fixture(scope="module")
def handles():
    """one batch handle per min_plateau, max_sym 1"""
    from wifirx import capi
    hs = {mp: capi.WifiRx(max_sym=1, min_plateau=mp) for mp in rows.PLATEAUS}
    yield hs
    for rx in hs.values():
        rx.close()


def check_cfo(cfo, Ar, Ai):
    """rule 1's bound on sp_atan2 (4e-7), one division by 16 (exact) and the rounding of the result"""
    want = np.arctan2(Ai.astype(np.float64), Ar.astype(np.float64)) / 16
    assert np.all(np.abs(cfo.astype(np.float64) - want) <= 4e-7 / 16 + 2.0 ** -24 * np.abs(cfo.astype(np.float64)))


def restated_slots(orc, slots, thr, mp):
    """(detected [n] bool, trigger [n], cfo_coarse [n], Ar, Ai) of the restatement, slot by slot"""
    n = len(slots)
    det, trig = np.zeros(n, bool), np.full(n, -1, np.int32)
    Ar, Ai = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for k, s in enumerate(slots):
        t, ar, ai = ref.detect(s, thr, mp, first_only=True)
        if len(t):
            det[k], trig[k], Ar[k], Ai[k] = True, t[0], ar[0], ai[0]
    cfo = np.where(det, orc.atan2(Ai, Ar) / F16, np.float32(0)).astype(np.float32)
    return det, trig, cfo, Ar, Ai


def oracle_slots(orc, slots, thr, mp):
    prm = orc.make_params(threshold=thr, min_plateau=mp, max_sym=1)
    out = np.zeros(len(slots), orc.FRAME_DTYPE)
    out["trigger"] = -1
    for k, s in enumerate(slots):
        if len(s):
            out[k] = orc.demod_batch(s, len(s), prm)["frames"][0]
    return out


@pytest.mark.parametrize("cls", rows.CLASSES)
@pytest.mark.parametrize("mp", rows.PLATEAUS)
def test_batch_rows(orc, handles, mp, cls):
    from wifirx import capi
    rx = handles[mp]
    n_det = 0
    for r in rows.batch_rows(mp, cls):
        slots = rows.slots_of(r)
        det, trig, cfo, Ar, Ai = restated_slots(orc, slots, r["thr"], mp)
        want = oracle_slots(orc, slots, r["thr"], mp)
        assert np.array_equal((want["flags"] & capi.F_DETECTED) != 0, det), r["name"]
        rx.set_param(capi.P_SENSITIVITY, r["thr"])
        d_iq = rx.alloc(max(r["x"].nbytes, 16)).upload(r["x"])
        for n in tuple(r.get("prefixes", ())) + (len(slots),):
            n = min(n, len(slots))
            fr = Fenced(rx, n, 32, off=0)
            dev = {"frames": _Ptr(fr.ptr)}
            if "off" in r:
                rx.demod_batch_var_dev(d_iq.ptr, r["off"][:n + 1], dev)
            else:
                rx.demod_batch_dev(d_iq.ptr, r["slot_len"], n, dev)
            rx.sync()
            raw = fr.download()
            got = raw[fr.at:fr.at + n * 32].view(capi.FRAME_DTYPE)
            assert np.array_equal((got["flags"] & capi.F_DETECTED) != 0, det[:n]), (r["name"], n)
            assert np.array_equal(got["trigger"], trig[:n]), (r["name"], n, got["trigger"], trig[:n])
            assert np.array_equal(u32(got["cfo_coarse"]), u32(cfo[:n])), (r["name"], n)
            check_cfo(got["cfo_coarse"][det[:n]], Ar[:n][det[:n]], Ai[:n][det[:n]])
            # the whole records are the oracle's, and no byte outside the n rows has changed
            assert np.array_equal(raw, fr.expected(want[:n].view(np.uint8))), (r["name"], n)
            fr.free()
        d_iq.free()
        n_det += int(det.sum())
    assert n_det > 10


def run_stream(x, mp, thr, chunk, batch, switch=None):
    """x through wifirx_push / wifirx_poll on a handle of its own; chunk 0: one push.  switch = (samples, thr): the
    sensitivity is set to thr once that many samples have been pushed.  Returns (frame records, passes of the pipeline)."""
    from wifirx import capi
    rx = capi.WifiRx(max_sym=1, min_plateau=mp, sensitivity=thr)
    rx.set_param(capi.P_STREAM_BATCH, batch)
    chunk = chunk or max(x.size, 1)
    got, pushed, k = [], 0, 0
    for p in range(0, x.size, chunk):
        if switch is not None and pushed == switch[0]:
            rx.set_param(capi.P_SENSITIVITY, switch[1])
        rx.push(x[p:p + chunk])
        pushed += x[p:p + chunk].size
        k += 1
        if k % 64 == 0 and rx.queued():
            got.append(rx.poll(cap=256)["frames"])
    rx.flush()
    while rx.queued():
        got.append(rx.poll(cap=256)["frames"])
    st = rx.stats()
    rx.close()
    assert st["samples_in"] == x.size
    passes = (k if not batch else x.size // batch) + 1
    return (np.concatenate(got) if got else np.zeros(0, capi.FRAME_DTYPE)), passes, st


def oracle_stream(orc, x, thr, mp):
    prm = orc.make_params(threshold=thr, min_plateau=mp, max_sym=1)
    o = orc.demod_stream(x, prm, cap=1024)
    orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
    return o["frames"]


@pytest.mark.parametrize("cls", rows.CLASSES)
@pytest.mark.parametrize("mp", rows.PLATEAUS)
def test_stream_rows(orc, mp, cls):
    """every push size and both WIFIRX_P_STREAM_BATCH values on the `sweep` stream (more than 40 000 samples: runs across
    push boundaries, tiles, wave spans, and -- more than two passes of at least 20 000 samples -- across the carry); two
    push sizes, rotating through the list, and both batch sizes on every other stream"""
    n_trig = 0
    for k, r in enumerate(rows.stream_rows(mp, cls)):
        x, thr = r["x"], r["thr"]
        t, Ar, Ai = ref.detect(x, thr, mp)
        cfo = (orc.atan2(Ai, Ar) / F16).astype(np.float32)
        want = oracle_stream(orc, x, thr, mp)
        assert np.array_equal(want["trigger"], t), r["name"]
        pushes = rows.PUSHES if r.get("sweep") else (rows.PUSHES[k % 9], rows.PUSHES[(k + 4) % 9])
        for chunk in pushes:
            for batch in rows.STREAM_BATCHES:
                got, passes, st = run_stream(x, mp, thr, chunk, batch)
                where = (r["name"], chunk, batch)
                assert np.array_equal(got["trigger"], t), (where, got["trigger"], t)
                assert np.array_equal(u32(got["cfo_coarse"]), u32(cfo)), where
                check_cfo(got["cfo_coarse"], Ar, Ai)
                assert np.array_equal(got, want), where
                assert st["frames_detected"] == len(t), where
                if r.get("sweep") and (chunk or batch):
                    # every pass but the last leaves more than the history behind it: the buffer moved more than once
                    # (one push of everything without a batch size is the one run with a single pass and the flush)
                    assert passes >= 3 and x.size > 2 * max(batch, chunk, 1024), where
        n_trig += len(t)
    assert n_trig > 10


@pytest.mark.parametrize("batch", [0, 5000])
@pytest.mark.parametrize("mp", rows.PLATEAUS)
def test_sensitivity_switched_between_pushes(orc, mp, batch):
    """WIFIRX_P_SENSITIVITY acts on every sample the detection has not run over: with batch size 0 on the samples of
    later pushes; with a batch size on the samples still staged as well (here 2432 of them, bursts included)"""
    x, staged_from, pushed = rows.switch_stream(mp)
    frontier = pushed if batch == 0 else staged_from
    assert batch == 0 or frontier == pushed // batch * batch
    Ar, Ai, P = ref.window_sums(x)
    for thr1, thr2 in ((0.5, rows.NEXT75), (rows.NEXT75, 0.5)):
        thr = np.where(np.arange(x.size) < frontier, np.float32(thr1), np.float32(thr2))
        t = np.asarray(ref.sync_short(ref.above(Ar, Ai, P, thr)[0], mp), dtype=np.int64)
        one = [ref.sync_short(ref.above(Ar, Ai, P, v)[0], mp) for v in (thr1, thr2)]
        assert list(t) not in one                       # the switch shows, and on both sides of it
        assert (t < frontier).any() and ((t >= frontier) & (t < pushed)).any() == (batch != 0) and (t >= pushed).any()
        cfo = (orc.atan2(Ai[t], Ar[t]) / F16).astype(np.float32)
        got, _, _ = run_stream(x, mp, thr1, 777, batch, switch=(pushed, thr2))
        assert np.array_equal(got["trigger"], t), (got["trigger"], t)
        assert np.array_equal(u32(got["cfo_coarse"]), u32(cfo))


def test_sensitivity_the_squared_comparison_cannot_honour_is_refused(orc, handles):
    from wifirx import block, capi
    r = [r for r in rows.batch_rows(2, "unit") if r["name"].startswith("thr/") and r["thr"] == 0.5][0]
    rx = capi.WifiRx(max_sym=1, min_plateau=2, sensitivity=0.5)
    for bad in (-rows.NEXT75, -1e-30, float("nan"), float("-inf")):
        with pytest.raises(capi.WifiRxError) as e:
            rx.set_param(capi.P_SENSITIVITY, bad)
        assert e.value.code == capi.EINVAL
    # the handle kept 0.5: |-nextafter(0.75, 0)| would trigger elsewhere
    got = rx.demod_batch(r["x"], r["slot_len"])["frames"]
    det, trig, cfo, _, _ = restated_slots(orc, rows.slots_of(r), 0.5, 2)
    other = restated_slots(orc, rows.slots_of(r), rows.NEXT75, 2)[1]
    assert np.array_equal(got["trigger"], trig) and not np.array_equal(trig, other)
    rx.set_param(capi.P_SENSITIVITY, 0.0)               # the edge of the domain is in it
    rx.close()
    for bad in (-0.5, float("nan")):
        with pytest.raises(capi.WifiRxError) as e:
            capi.WifiRx(sensitivity=bad)
        assert e.value.code == capi.EINVAL
    b = block.wifi_phy_rx(bandwidth=20e6, frequency=5.89e9, sensitivity=0.56, chan_est=block.LS)
    with pytest.raises(capi.WifiRxError):
        b.set_sensitivity(-0.56)
    assert b.get_sensitivity() == 0.56
    b.set_sensitivity(0.6)
    assert b.get_sensitivity() == 0.6
    with pytest.raises(capi.WifiRxError):
        block.wifi_phy_rx(sensitivity=-0.56)
