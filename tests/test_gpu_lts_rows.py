"""Frame synchronisation on the device, on the host-built rows of tests/lts_rows.py: the coarse derotation, the two-stage
LTS search, the pair search and the fine CFO (preamble_load .. preamble_pair_finish of csrc/wr_quad.h) through
wifirx_demod_batch / _v in every arrangement of the table -- a row's record must not depend on its place in a wave or on
its neighbour -- and through wifirx_push / wifirx_poll for every chunking, against the restatement of tests/lts_ref.py
(SYNC, frame_start, the bits of cfo_fine) and against the oracle's whole records.  Equality throughout."""
import numpy as np
import pytest

import lts_rows as rows
from helpers import Fenced

pytestmark = pytest.mark.gpu

V_NEVER = 200               # length of the never-triggering slot in the variable-length form


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr


@pytest.fixture(scope="module")
def rx():
    from wifirx import capi
    h = capi.WifiRx(max_sym=1, min_plateau=rows.MP, sensitivity=rows.THR)
    yield h
    h.close()


_want = {}


def slot_samples(entry, form):
    if isinstance(entry, str):
        if entry == "empty":
            assert form == "v"
            return np.zeros(0, np.complex64)
        return rows.never_slot(rows.SLOT if form == "u" else V_NEVER)
    return rows.slot_of(entry, rows.SLOT if form == "u" else None)


def want_of(orc, entry, form, chan_est=0):
    """(oracle record, restated record) of one entry as a slot of the form: the same wherever it stands"""
    key = (entry if isinstance(entry, str) else entry["name"], form, chan_est)
    if key not in _want:
        x = slot_samples(entry, form)
        rec = np.zeros(1, orc.FRAME_DTYPE)
        rec["trigger"] = -1
        f = dict(t=-1, flags=0, frame_start=0, cfo_fine=np.float32(0))
        if x.size:
            thr, mp = (rows.THR, rows.MP) if isinstance(entry, str) else (entry["thr"], entry["mp"])
            rec[0] = orc.demod_batch(x, x.size, orc.make_params(threshold=thr, min_plateau=mp, max_sym=1, chan_est=chan_est))["frames"][0]
            if not isinstance(entry, str):
                f = rows.restate(entry, orc.sincos, orc.atan2, (), rows.SLOT if form == "u" else None)
        _want[key] = (rec[0], f)
    return _want[key]


def check(orc, got, raw, fr, entries, form, where, chan_est=0):
    from wifirx import capi
    want = np.array([want_of(orc, e, form, chan_est)[0] for e in entries], dtype=orc.FRAME_DTYPE)
    for k, e in enumerate(entries):
        f = want_of(orc, e, form, chan_est)[1]
        name = e if isinstance(e, str) else e["name"]
        assert got["trigger"][k] == f["t"], (where, k, name)
        keep = capi.F_DETECTED | capi.F_SYNC
        assert (int(got["flags"][k]) & keep, int(got["frame_start"][k]), int(u32(got["cfo_fine"][k])[0])) == \
            (int(f["flags"]) & keep, int(f["frame_start"]), int(u32(f["cfo_fine"])[0])), (where, k, name, got[k], f["frame_start"], f["cfo_fine"])
    bad = [(k, entries[k] if isinstance(entries[k], str) else entries[k]["name"]) for k in np.flatnonzero(got != want)]
    assert not bad, (where, bad[:8], got[bad[0][0]], want[bad[0][0]])
    if raw is not None:         # no byte outside the n records has changed
        assert np.array_equal(raw, fr.expected(want.view(np.uint8))), where


def run_dev(orc, h, entries, form, where, chan_est=0):
    from wifirx import capi
    parts = [slot_samples(e, form) for e in entries]
    x = np.concatenate(parts)
    n = len(entries)
    d_iq = h.alloc(max(x.nbytes, 16)).upload(x)
    fr = Fenced(h, n, 32, off=0)
    dev = {"frames": _Ptr(fr.ptr)}
    if form == "u":
        h.demod_batch_dev(d_iq.ptr, rows.SLOT, n, dev)
    else:
        h.demod_batch_var_dev(d_iq.ptr, np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64), dev)
    h.sync()
    raw = fr.download()
    got = raw[fr.at:fr.at + n * 32].view(capi.FRAME_DTYPE)
    try:
        check(orc, got, raw, fr, entries, form, (where, form), chan_est)
    finally:
        fr.free()
        d_iq.free()


ARR = dict(rows.arrangements())


def test_each_row_alone(orc, rx):
    for r in rows.main_rows():
        for form in "uv":
            run_dev(orc, rx, [r], form, "alone/" + r["name"])


@pytest.mark.parametrize("name", [n for n in ARR if not n.startswith("alone/")])
def test_arrangements(orc, rx, name):
    """table order (the last wave holds one row), reversed, rotated by 1, 2, 3; every row in both places of a pair and in
    both pairs of a wave beside a shortcut row, a wide-path row, a row with L < 383, a slot that never triggers and a
    slot of length 0"""
    for form in "uv":
        if form == "u" and name == "beside_empty":
            continue                        # uniform slots have one length
        run_dev(orc, rx, ARR[name], form, name)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 9])
def test_last_wave_not_full(orc, rx, n):
    ent = ARR["reversed"][:n]
    for form in "uv":
        run_dev(orc, rx, ent, form, "prefix%d" % n)


@pytest.mark.parametrize("chan_est", [0, 1, 2, 3])
def test_four_equalisers(orc, chan_est):
    """the preamble code is shared, the kernel instances are not: table order under LS, LMS, COMB and STA"""
    from wifirx import capi
    h = capi.WifiRx(max_sym=1, min_plateau=rows.MP, sensitivity=rows.THR, chan_est=chan_est)
    try:
        for form in "uv":
            run_dev(orc, h, ARR["order"], form, "eq%d" % chan_est, chan_est)
    finally:
        h.close()


def test_host_iq(orc, rx):
    """the same records from samples in host memory (wifirx_demod_batch and _v with iq_on_device = 0)"""
    ent = ARR["rotated2"]
    got = rx.demod_batch(np.concatenate([slot_samples(e, "u") for e in ent]), rows.SLOT)["frames"]
    check(orc, got, None, None, ent, "u", "host/u")
    ent = ARR["beside_empty"][:64]
    parts = [slot_samples(e, "v") for e in ent]
    got = rx.demod_batch_var(np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]))["frames"]
    check(orc, got, None, None, ent, "v", "host/v")


def test_earliest_trigger(orc):
    """t = 16 and 17: the single-pointer load needs t >= 16 (threshold 0 and min_plateau 0 / 1: handles of their own)"""
    from wifirx import capi
    seen = set()
    for r in rows.table():
        if (r["thr"], r["mp"]) == (rows.THR, rows.MP):
            continue
        h = capi.WifiRx(max_sym=1, min_plateau=r["mp"], sensitivity=r["thr"])
        try:
            run_dev(orc, h, [r], "v", r["name"])
            run_dev(orc, h, [r, r, r], "v", r["name"])
            seen.add(want_of(orc, r, "v")[1]["t"])
        finally:
            h.close()
    assert seen == {16, 17}


# ---- stream mode ------------------------------------------------------------------------------------------------------

def run_stream(x, chunks, batch):
    """x through wifirx_push / wifirx_poll on a handle of its own, cut into `chunks` samples (the rest in one push), then
    a flush"""
    from wifirx import capi
    h = capi.WifiRx(max_sym=1, min_plateau=rows.MP, sensitivity=rows.THR)
    h.set_param(capi.P_STREAM_BATCH, batch)
    got, p, k = [], 0, 0
    for c in list(chunks) + [x.size]:
        c = min(c, x.size - p)
        if c <= 0:
            break
        h.push(x[p:p + c])
        p += c
        k += 1
        if k % 64 == 0 and h.queued():
            got.append(h.poll(cap=256)["frames"])
    h.flush()
    while h.queued():
        got.append(h.poll(cap=256)["frames"])
    st = h.stats()
    h.close()
    assert st["samples_in"] == x.size
    return np.concatenate(got) if got else np.zeros(0, capi.FRAME_DTYPE)


_streams = {}


def stream_want(orc, key, x):
    """(oracle's stream records, restated records) of a stream, computed once"""
    if key not in _streams:
        prm = orc.make_params(threshold=rows.THR, min_plateau=rows.MP, max_sym=1)
        o = orc.demod_stream(x, prm, cap=1024)
        orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
        _streams[key] = (o["frames"], rows.restate_stream(x, rows.THR, rows.MP, orc.sincos, orc.atan2))
    return _streams[key]


def check_stream(orc, got, key, x, where, n_rows=None):
    from wifirx import capi
    want, fs = stream_want(orc, key, x)
    assert len(fs) == len(want) and (n_rows is None or len(fs) == n_rows), (where, len(fs), len(want), n_rows)
    assert len(got) == len(want), (where, len(got), len(want))
    keep = capi.F_DETECTED | capi.F_SYNC
    for k, f in enumerate(fs):
        assert got["trigger"][k] == f["t"], (where, k)
        assert (int(got["flags"][k]) & keep, int(got["frame_start"][k]), int(u32(got["cfo_fine"][k])[0])) == \
            (int(f["flags"]) & keep, int(f["frame_start"]), int(u32(f["cfo_fine"])[0])), (where, k, got[k], f["frame_start"], f["cfo_fine"])
    bad = np.flatnonzero(got != want)
    assert not bad.size, (where, bad[:8], got[bad[0]], want[bad[0]])


SETS = dict(rows.stream_sets())


@pytest.mark.parametrize("chunk", rows.PUSHES)
@pytest.mark.parametrize("name", list(SETS))
def test_stream_rows(orc, name, chunk):
    """the rows 700 exact zeros apart (one trigger each, where the row's burst ends), every push size, both batch sizes"""
    x, starts = rows.stream_of(SETS[name])
    for batch in rows.STREAM_BATCHES:
        got = run_stream(x, [chunk] * (x.size // chunk) if chunk else [], batch)
        check_stream(orc, got, name, x, (name, chunk, batch), n_rows=len(starts))
    fs = stream_want(orc, name, x)[1]
    # one trigger per row: on the integer burst's last sample exactly, in the preamble rows inside the short training field
    for f, s, r in zip(fs, starts, SETS[name]):
        assert f["t"] == s + rows.LB - 1 if r["ints"] else s <= f["t"] < s + 140, (name, r["name"], f["t"], s)


@pytest.mark.parametrize("name", list(SETS))
def test_stream_cut_inside_the_window(orc, name):
    """a push ends just behind the trigger, in the middle of the window, and at window index 382 / 383 / 384 of every
    row in turn: the trigger is carried to the next push with its coarse CFO"""
    x, starts = rows.stream_of(SETS[name])
    fs = stream_want(orc, name, x)[1]
    for batch in rows.STREAM_BATCHES:
        for shift in range(2):
            cuts = []
            for k, f in enumerate(fs):
                w0 = f["t"] - 16                    # stream index of window index 0
                cuts += [(f["t"] + 1,), (w0 + 200,), (w0 + 382,), (w0 + 383,), (w0 + 384,), (f["t"] + 1, w0 + 383, w0 + 384)][(k + 3 * shift) % 6]
            pos = [0] + sorted(set(cuts))
            got = run_stream(x, np.diff(pos), batch)
            check_stream(orc, got, name, x, (name, "cuts", shift, batch), n_rows=len(starts))


@pytest.mark.parametrize("L", [382, 383, 384, 385])
def test_stream_ends_inside_the_last_window(orc, L):
    """the stream ends where the last row has L samples, then a flush: 382 is TRUNCATED, 383 the smallest window that
    still searches (sample 383 is a zero), 384 ends on the window's last sample"""
    from wifirx import capi
    by = {r["name"]: r for r in rows.main_rows()}
    ent = [by["pair/64"], by["shortcut/above"], by["pair/lag319"]]
    x, starts = rows.stream_of(ent, last_L=L)
    for batch in rows.STREAM_BATCHES:
        for chunks in ([], [777] * (x.size // 777), [x.size - 1], [x.size - 2]):
            got = run_stream(x, chunks, batch)
            check_stream(orc, got, ("end", L), x, ("end", L, batch, len(chunks)), n_rows=3)
            assert bool(got["flags"][2] & capi.F_SYNC) == (L >= 383) and bool(got["flags"][0] & capi.F_SYNC)
