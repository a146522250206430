"""The symbol path on the device, on the host-built rows of tests/symbol_rows.py: the SIGNAL symbol and its packed
four-frame Viterbi (viterbi_signal4), parse_signal, the data-symbol bookkeeping and the slicer with its LLR stores
(csrc/wr_quad.h) through wifirx_demod_batch / _v for every output set -- the plain kernels and their constellation loops,
the kernels that also deliver the equalised points, bf16 LLRs, the bit planes alone, llr_csi 1 -- under the four
equalisers, and through wifirx_push / wifirx_poll for every chunking.  The device must equal the oracle's whole records
and outputs bit for bit, and the restatement of tests/symbol_ref.py applied to the constructed SIGNAL bits and to the
device's OWN equalised points.  Every output lies in a fenced buffer filled with a canary: nothing is written behind a
frame's n_sym_out symbols, and nothing for a slot without a frame."""
import numpy as np
import pytest

import symbol_ref as ref
import symbol_rows as rows
from helpers import FILL, Fenced
from llr_bf16_ref import bf16_rne, bf16_to_f32

pytestmark = pytest.mark.gpu

EQS = (0, 1, 2, 3)
# name -> (want_carrier, llr format, outputs handed to the call, llr_csi)
SETS = {
    "plain": (False, "f32", ("idx", "llr"), 0),
    "carrier": (True, "f32", ("idx", "llr", "carrier", "hbits"), 0),
    "bf16": (False, "bf16", ("idx", "llr"), 0),
    "carrier_bf16": (True, "bf16", ("idx", "llr", "carrier"), 0),
    "planes": (False, "f32", ("hbits",), 0),
    "csi": (False, "f32", ("idx", "llr", "hbits"), 1),
    "carrier_csi": (True, "f32", ("idx", "llr", "carrier", "csi"), 1),
}


class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr


def make_handle(grp, chan_est=0, set_name="plain"):
    from wifirx import capi
    car, fmt, _, csi = SETS[set_name]
    h = capi.WifiRx(max_sym=rows.GROUPS[grp]["max_sym"], llr_bits=rows.LLR_BITS, chan_est=chan_est, want_carrier=car, llr_format=fmt)
    if csi:
        h.set_param(capi.P_LLR_CSI, 1)
    return h


def row_bytes(kind, ms, fmt):
    return {"frames": 32, "idx": ms * 48, "llr": ms * 48 * rows.LLR_BITS * (2 if fmt == "bf16" else 4), "carrier": ms * 48 * 8,
            "hbits": ms * 48, "csi": 52 * 8}[kind]


def expected_rows(orc, entries, form, grp, chan_est, set_name):
    """kind -> uint8 [n, row bytes]: what the oracle says each output row holds, FILL where nothing may be written"""
    _, fmt, kinds, csi = SETS[set_name]
    ms = rows.GROUPS[grp]["max_sym"]
    n = len(entries)
    out = {k: np.full((n, row_bytes(k, ms, fmt)), FILL, np.uint8) for k in ("frames",) + kinds}
    for k, e in enumerate(entries):
        o = rows.expected(orc, e, form, chan_est, csi, grp)
        fr = np.array([o["frame"]], dtype=orc.FRAME_DTYPE)
        if "llr" not in kinds:
            fr["flags"] &= ~np.uint32(orc.F_LLR)                    # no LLR buffer, no LLRs
        out["frames"][k] = fr.view(np.uint8)
        no, nb = int(fr["n_sym_out"][0]), int(fr["n_bpsc"][0])
        if "idx" in kinds:
            out["idx"][k, :no * 48] = o["idx"][:no].reshape(-1)
        if "carrier" in kinds:
            out["carrier"][k, :no * 48 * 8] = o["eq"][:no].reshape(-1).view(np.uint8)
        if "llr" in kinds and fr["flags"][0] & orc.F_LLR:
            v = o["llr"][:no * 48 * nb]
            v = bf16_rne(v) if fmt == "bf16" else v
            out["llr"][k, :v.nbytes] = v.view(np.uint8)
        if "hbits" in kinds:
            w = ref.planes(o["idx"], nb, no, ms)[:no * 2 * nb]
            out["hbits"][k, :w.nbytes] = w.view(np.uint8)
        if "csi" in kinds and fr["flags"][0] & orc.F_SYNC:
            out["csi"][k] = o["csi"].view(np.uint8)
    return out


def float_rows_differ(got, want, bf16):
    """raw bytes of one row of float32 / bf16 values: None if equal -- NaN by position, everything else (the canary
    included: it is no NaN in either format) by its bits --, else what differs"""
    dt = np.uint16 if bf16 else np.uint32
    g, w = np.ascontiguousarray(got).view(dt), np.ascontiguousarray(want).view(dt)
    gn, wn = (np.isnan(bf16_to_f32(v)) if bf16 else np.isnan(v.view(np.float32)) for v in (g, w))
    if not np.array_equal(gn, wn):
        return "NaN at element %d of one side only" % int(np.flatnonzero(gn != wn)[0])
    d = np.flatnonzero((g != w) & ~wn)
    return None if not d.size else "element %d: %#x, expected %#x" % (int(d[0]), int(g[d[0]]), int(w[d[0]]))


def check_restated(orc, entries, form, grp, frames, car, idx, llr, csi, fmt, llr_csi, where, llr_bits):
    """tests/symbol_ref.py on the constructed bits and on the device's own points"""
    g = rows.GROUPS[grp]
    for k, e in enumerate(entries):
        if isinstance(e, str):
            assert not int(frames["flags"][k]) & (ref.F_SIGNAL | orc.F_SYNC), (where, k, e)
            continue
        fr = frames[k]
        assert fr["flags"] & orc.F_SYNC, (where, k, e["name"])
        want = rows.restated_record(e, fr, rows.entry_samples(e, form, grp).size, g["max_sym"], (), llr_bits)
        assert rows.record_tuple(fr) == rows.record_tuple(want), (where, k, e["name"], fr, want)
        no, nb = int(fr["n_sym_out"]), int(fr["n_bpsc"])
        if car is None or not no:
            continue
        Y = car[k, :no]
        assert np.array_equal(ref.decide(Y, nb), idx[k, :no]), (where, k, e["name"])
        L = ref.llr_weighted(Y, nb, ref.weight(csi[k])) if llr_csi else ref.llr(Y, nb)
        got = llr[k, :no * 48 * nb]
        if fmt == "bf16":
            wb = bf16_rne(L.reshape(-1))
            nan = np.isnan(L.reshape(-1))
            assert np.array_equal(np.isnan(bf16_to_f32(got)), nan) and np.array_equal(got[~nan], wb[~nan]), (where, k, e["name"])
        else:
            nan = np.isnan(L.reshape(-1))
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], L.reshape(-1).view(np.uint32)[~nan]), (where, k, e["name"])


def run_dev(orc, h, entries, form, grp, chan_est, set_name, where):
    from wifirx import capi
    _, fmt, kinds, llr_csi = SETS[set_name]
    ms = rows.GROUPS[grp]["max_sym"]
    parts = [rows.entry_samples(e, form, grp) for e in entries]
    x = np.concatenate(parts)
    n = len(entries)
    d_iq = h.alloc(max(x.nbytes, 16)).upload(x)
    fences = {k: Fenced(h, n, row_bytes(k, ms, fmt)) for k in ("frames",) + kinds}
    dev = {k: _Ptr(f.ptr) for k, f in fences.items()}
    try:
        if form == "u":
            h.demod_batch_dev(d_iq.ptr, rows.GROUPS[grp]["slot"], n, dev)
        else:
            h.demod_batch_var_dev(d_iq.ptr, np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64), dev)
        h.sync()
        want = expected_rows(orc, entries, form, grp, chan_est, set_name)
        got = {}
        for k, f in fences.items():
            raw = f.download()
            assert np.all(raw[:f.at] == FILL) and np.all(raw[f.at + n * f.stride:] == FILL), (where, k, "fence")
            got[k] = raw[f.at:f.at + n * f.stride].reshape(n, f.stride)
        frames = got["frames"].reshape(-1).view(capi.FRAME_DTYPE)
        wf = want["frames"].reshape(-1).view(capi.FRAME_DTYPE)
        bad = [(k, rows.entry_name(entries[k])) for k in np.flatnonzero(frames != wf)]
        assert not bad, (where, bad[:8], frames[bad[0][0]], wf[bad[0][0]])
        for k in kinds:
            if k in ("llr", "carrier", "csi"):
                for i in range(n):
                    d = float_rows_differ(got[k][i], want[k][i], k == "llr" and fmt == "bf16")
                    assert d is None, (where, k, i, rows.entry_name(entries[i]), d)
            else:
                rb = np.flatnonzero((got[k] != want[k]).any(axis=1))
                assert not rb.size, (where, k, [(int(i), rows.entry_name(entries[i])) for i in rb[:8]],
                                     "first differing byte", int(np.flatnonzero(got[k][rb[0]] != want[k][rb[0]])[0]))
        idx = got["idx"].reshape(n, ms, 48) if "idx" in kinds else None
        car = got["carrier"].reshape(-1).view(np.complex64).reshape(n, ms, 48) if "carrier" in kinds and "idx" in kinds else None
        llr = got["llr"].reshape(n, -1).view(np.uint16 if fmt == "bf16" else np.float32) if "llr" in kinds else None
        csi = got["csi"].reshape(-1).view(np.complex64).reshape(n, 52) if "csi" in kinds else None
        if llr_csi and csi is None:
            car = None
        check_restated(orc, entries, form, grp, frames, car, idx, llr, csi, fmt, llr_csi, where, rows.LLR_BITS if "llr" in kinds else 0)
    finally:
        for f in fences.values():
            f.free()
        d_iq.free()


def forms_of(entries):
    return "uv" if "empty" not in entries else "v"


@pytest.mark.parametrize("chan_est", EQS)
@pytest.mark.parametrize("set_name", list(SETS))
def test_every_group_every_output_set(orc, set_name, chan_est):
    """every row of the table in table order, uniform and variable-length slots"""
    for grp in rows.GROUPS:
        h = make_handle(grp, chan_est, set_name)
        try:
            for form in "uv":
                run_dev(orc, h, rows.group(grp), form, grp, chan_est, set_name, (grp, set_name, chan_est, form))
        finally:
            h.close()


ARR = dict(rows.sig_arrangements())


@pytest.mark.parametrize("set_name", ["plain", "carrier"])
@pytest.mark.parametrize("name", [n for n in ARR if n != "order"])
def test_signal_rows_in_every_place_of_a_wave(orc, name, set_name):
    """the SIGNAL rows reversed, rotated by 1, 2 and 3; four classes in one register in every rotation; the worst-metric
    word beside the all-zero word in every byte; last waves of 1, 2 and 3 rows; beside a slot that never triggers and a slot
    of length 0: a row's record does not depend on its byte of the packed registers or on its neighbours"""
    h = make_handle("sig", 0, set_name)
    try:
        for form in forms_of(ARR[name]):
            run_dev(orc, h, ARR[name], form, "sig", 0, set_name, (name, set_name, form))
    finally:
        h.close()


@pytest.mark.parametrize("chan_est", EQS)
def test_mixed_rates_in_one_wave(orc, chan_est):
    """the claimed-rate rows and the threshold rows of all four constellations interleaved: waves whose rows differ in
    constellation, length and in whether they go on"""
    T = rows.group("thr")
    by = rows.by_name()
    ent = []
    for k in range(8):
        ent += [by["claim/enc%d" % k], by["thr/nb1/%d" % (k % 6)], by["claim/enc%d" % (7 - k)], by["thr/nb4/%d" % k]]
    ent += [T[k] for k in np.random.default_rng(3).permutation(len(T))]
    for set_name in ("plain", "carrier", "csi", "bf16"):
        h = make_handle("thr", chan_est, set_name)
        try:
            for form in "uv":
                run_dev(orc, h, ent, form, "thr", chan_est, set_name, ("mixed", set_name, chan_est, form))
        finally:
            h.close()


def test_host_samples(orc):
    """the same outputs from samples in host memory (wifirx_demod_batch and _v with iq_on_device = 0)"""
    from wifirx import capi
    for grp, ent in (("sig", ARR["rotated2"]), ("thr", rows.group("thr"))):
        g = rows.GROUPS[grp]
        h = capi.WifiRx(max_sym=g["max_sym"], llr_bits=rows.LLR_BITS, want_carrier=True)
        try:
            for form in "uv":
                parts = [rows.entry_samples(e, form, grp) for e in ent]
                if form == "u":
                    r = h.demod_batch(np.concatenate(parts), g["slot"])
                else:
                    r = h.demod_batch_var(np.concatenate(parts), np.concatenate([[0], np.cumsum([p.size for p in parts])]))
                for k, e in enumerate(ent):
                    o = rows.expected(orc, e, form, 0, 0, grp)
                    no, nb = int(o["frame"]["n_sym_out"]), int(o["frame"]["n_bpsc"])
                    assert r["frames"][k] == o["frame"], (grp, form, k, rows.entry_name(e), r["frames"][k], o["frame"])
                    assert np.array_equal(r["idx"][k, :no], o["idx"][:no]), (grp, form, k)
                    assert np.array_equal(r["carrier"][k, :no].view(np.uint32), o["eq"][:no].view(np.uint32)), (grp, form, k)
                    assert np.array_equal(r["llr"][k, :no * 48 * nb].view(np.uint32), o["llr"][:no * 48 * nb].view(np.uint32)), (grp, form, k)
        finally:
            h.close()


# ---- decode_mac ---------------------------------------------------------------------------------------------------------

def test_decode_mac_on_the_rows_that_complete(orc, decode_path):
    """the SIGNAL rows with n_sym <= max_sym, LENGTH 0 and 3 among them (shorter than a frame check sequence: DECODED
    without CRC_OK): records and PSDU bytes as the oracle's decode_mac leaves them"""
    from wifirx import capi
    g = rows.GROUPS["sig"]
    ent = [r for r in rows.group("sig") if rows.expected(orc, r, "u")["frame"]["flags"] & orc.F_COMPLETE]
    lens = {int(rows.expected(orc, r, "u")["frame"]["psdu_len"]) for r in ent}
    assert {0, 1, 3, 4} <= lens and len(ent) >= 20
    ent = ent + [rows.by_name()["field/len4095/enc0"], rows.by_name()["field/parity_wrong/9"]]
    x = np.concatenate([rows.entry_samples(e, "u", "sig") for e in ent])
    h = capi.WifiRx(max_sym=g["max_sym"], llr_bits=rows.LLR_BITS)
    try:
        r = h.demod_batch(x, g["slot"], decode=True, psdu_stride=256)
    finally:
        h.close()
    prm = orc.make_params(max_sym=g["max_sym"], llr_bits=rows.LLR_BITS)
    frames = np.array([rows.expected(orc, e, "u")["frame"] for e in ent], dtype=orc.FRAME_DTYPE)
    idx = np.stack([rows.expected(orc, e, "u")["idx"] for e in ent])
    psdu = orc.decode_batch(frames, idx, prm, psdu_stride=256)
    bad = np.flatnonzero(r["frames"] != frames)
    assert not bad.size, (decode_path, [(int(k), ent[k]["name"]) for k in bad[:8]], r["frames"][bad[0]], frames[bad[0]])
    for k, e in enumerate(ent):
        n = int(frames["psdu_len"][k]) if frames["flags"][k] & orc.F_DECODED else 0
        assert np.array_equal(r["psdu"][k, :n], psdu[k, :n]), (decode_path, e["name"])
        if n < 4:
            assert not frames["flags"][k] & orc.F_CRC_OK


# ---- stream mode --------------------------------------------------------------------------------------------------------

def stream_rows():
    """a stream's worth of the SIGNAL rows: every field class once, the four plain words, the searched words, a dozen random
    words; n_sym <= max_sym, n_sym > max_sym and failing SIGNAL words follow each other"""
    by = rows.by_name()
    names = ["field/rate%d" % k for k in (11, 15, 10, 5, 0, 8)] + ["field/parity_wrong/9", "field/reserved/12", "field/tail/63",
             "field/len0/enc0", "field/len3/enc7", "field/len4095/enc0", "field/len1529/enc7", "field/step3/enc2/lo", "field/step3/enc2/hi",
             "field/step3/enc6/hi", "far/zeros", "far/ones", "far/alt01", "far/period4", "far/searched/tie0", "far/searched/path",
             "far/searched/top"] + ["far/random/%d" % k for k in range(12)]
    return [by[n] for n in names]


def run_stream(x, chunks, batch, max_sym):
    from wifirx import capi
    h = capi.WifiRx(max_sym=max_sym, llr_bits=0)
    h.set_param(capi.P_STREAM_BATCH, batch)
    got, idx, p, k = [], [], 0, 0
    try:
        for c in list(chunks) + [x.size]:
            c = min(c, x.size - p)
            if c <= 0:
                break
            h.push(x[p:p + c])
            p += c
            k += 1
            if k % 64 == 0 and h.queued():
                r = h.poll(cap=256, psdu_stride=256, want_idx=True)
                got.append(r["frames"])
                idx.append(r["idx"])
        h.flush()
        while h.queued():
            r = h.poll(cap=256, psdu_stride=256, want_idx=True)
            got.append(r["frames"])
            idx.append(r["idx"])
        st = h.stats()
    finally:
        h.close()
    assert st["samples_in"] == x.size
    return (np.concatenate(got), np.concatenate(idx)) if got else (np.zeros(0, capi.FRAME_DTYPE), np.zeros((0, max_sym, 48), np.uint8))


_streams = {}


def stream_want(orc, x, max_sym):
    if "w" not in _streams:
        prm = orc.make_params(max_sym=max_sym)
        o = orc.demod_stream(x, prm, cap=1024)
        orc.decode_batch(o["frames"], o["idx"], prm, psdu_stride=2048)
        _streams["w"] = (o["frames"], o["idx"])
    return _streams["w"]


def check_stream(orc, got, x, R, starts, max_sym, where):
    frames, idx = got
    want, widx = stream_want(orc, x, max_sym)
    assert len(want) == len(R) and len(frames) == len(want), (where, len(frames), len(want), len(R))
    bad = np.flatnonzero(frames != want)
    assert not bad.size, (where, [(int(k), R[k]["name"]) for k in bad[:8]], frames[bad[0]], want[bad[0]])
    for k, r in enumerate(R):
        no = int(want["n_sym_out"][k])
        assert np.array_equal(idx[k, :no], widx[k, :no]), (where, k, r["name"])
        # the restatement: the record from the constructed bits; every row has all its samples, so only max_sym truncates
        w = ref.record(r["sig48"], 540 * 80, int(frames["frame_start"][k]), max_sym, 0)
        assert rows.record_tuple(frames[k]) == rows.record_tuple(w), (where, k, r["name"], frames[k], w)


@pytest.mark.parametrize("chunk", rows.PUSHES)
def test_stream_rows(orc, chunk):
    """the rows 700 exact zeros apart, every push size, both batch sizes: a record does not depend on where a push ends, and
    a row whose n_sym exceeds max_sym settles as the oracle's stream driver settles it"""
    R = stream_rows()
    ms = rows.GROUPS["sig"]["max_sym"]
    x, starts = rows.stream_of(R)
    for batch in rows.STREAM_BATCHES:
        got = run_stream(x, [chunk] * (x.size // chunk) if chunk else [], batch, ms)
        check_stream(orc, got, x, R, starts, ms, (chunk, batch))


def test_stream_push_ends_inside_the_signal_symbol(orc):
    """a push ends behind the preamble, inside the SIGNAL symbol's cyclic prefix, in the middle of its 64 samples, on its
    last sample and inside the first data symbol of every row in turn"""
    R = stream_rows()
    ms = rows.GROUPS["sig"]["max_sym"]
    x, starts = rows.stream_of(R)
    for batch in rows.STREAM_BATCHES:
        for shift in range(2):
            cuts = []
            for k, s in enumerate(starts):
                cuts += [(s + 320,), (s + 328,), (s + 336 + 30,), (s + 399,), (s + 400,), (s + 336 + 30, s + 400 + 50)][(k + 3 * shift) % 6]
            pos = [0] + sorted(set(cuts))
            got = run_stream(x, np.diff(pos), batch, ms)
            check_stream(orc, got, x, R, starts, ms, ("cuts", shift, batch))
