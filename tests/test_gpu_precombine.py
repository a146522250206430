"""wifirx_precombine (wr_precombine.hip) on the device: bit for bit against tests/precombine_ref.py on the rows of
tests/precombine_rows.py (every clause of NUMERICS.md rule 33, outputs between sentinels), its place on the stream in front of
the demod, the host conveniences, the refused arguments, and what it is for: fewer lost frames than the antennas alone at two
antennas, and no more than rule 23's maximal-ratio combining of four demods at a quarter of the demod work."""
import ctypes as C
import math

import numpy as np
import pytest

import precombine_point as pt
import precombine_ref as pr
import precombine_rows as rows
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256                     # sentinel bytes behind every output
N = 37


@pytest.fixture(scope="module")
def rx():
    """max_batch 64 for the range check"""
    r = capi.WifiRx(max_sym=txgen.n_sym_for(40, 0), llr_bits=6, want_carrier=True, max_batch=64, device=0)
    yield r
    r.close()


class Outputs:
    """y, weights and stats of one call on the device, each with GUARD sentinel bytes behind it"""

    def __init__(self, rx, n_ant, slot_len, n_slots):
        self.sizes = dict(y=n_slots * slot_len * 8, w=n_slots * n_ant * 8, s=n_slots * 16)
        self.fresh = {k: np.full(v + GUARD, FILL, np.uint8) for k, v in self.sizes.items()}
        self.dev = {k: rx.alloc(v.nbytes) for k, v in self.fresh.items()}
        self.shape = (n_ant, slot_len, n_slots)
        self.refill()

    def refill(self):
        for k, v in self.fresh.items():
            self.dev[k].upload(v)

    def download(self):
        return {k: self.dev[k].download(np.uint8, v.nbytes) for k, v in self.fresh.items()}

    def untouched(self, got, keys=("y", "w", "s")):
        return all(np.array_equal(got[k], self.fresh[k]) for k in keys)

    def split(self, got, n_slots):
        """(y, weights, stats) of the first n_slots slots, and whether every byte behind them still holds the sentinel"""
        A, S, _ = self.shape
        used = dict(y=n_slots * S * 8, w=n_slots * A * 8, s=n_slots * 16)
        clean = all((got[k][used[k]:] == FILL).all() for k in used)
        return (got["y"][:used["y"]].view(np.complex64).reshape(n_slots, S), got["w"][:used["w"]].view(np.complex64).reshape(n_slots, A),
                got["s"][:used["s"]].view(capi.PRE_STATS_DTYPE)), clean

    def free(self):
        for b in self.dev.values():
            b.free()


def agrees(got, want, xs):
    """y, weights and stats equal the reference's bit for bit (any NaN for any NaN), and a degenerate slot is antenna 0's bytes"""
    (y, w, s), (ry, rw, rs) = got, want
    if not (rows.same_values(y, ry) and rows.same_values(w, rw) and rows.same_values(s, rs)):
        return False
    deg = (s["flags"] & capi.PRE_DEGENERATE) != 0
    return rows.same_bits(y[deg], xs[0][:len(y)][deg])


@pytest.mark.parametrize("slot_len", (64, 128, 320, 1472))
@pytest.mark.parametrize("n_ant", (1, 2, 3, 8))
def test_rows_equal_the_reference(rx, n_ant, slot_len):
    """every case of precombine_rows, iters 0 / 1 / 4, 37 slots and the first slot alone (the bits of a slot do not depend on
    the batch: the one-slot call is held against slot 0 of the 37-slot reference)"""
    out = Outputs(rx, n_ant, slot_len, N)
    try:
        for case in rows.CASES:
            xs = rows.build(case, n_ant, slot_len, N)
            ins = [rx.alloc(x.nbytes).upload(x) for x in xs]
            try:
                for iters in (0, 1, 4):
                    want = pr.combine(xs, slot_len, iters)
                    for n in (N, 1):
                        out.refill()
                        rx.precombine_dev([b.ptr for b in ins], slot_len, n, out.dev["y"].ptr, iters, out.dev["w"].ptr, out.dev["s"].ptr)
                        rx.sync()
                        got, clean = out.split(out.download(), n)
                        assert clean, (case, iters, n)
                        assert agrees(got, tuple(v[:n] for v in want), xs), (case, iters, n)
            finally:
                for b in ins:
                    b.free()
    finally:
        out.free()


def test_the_cases_meet_their_clauses_on_the_device(rx):
    """the clauses themselves, read off the device's outputs (three antennas, 128 samples)"""
    A, S = 3, 128
    out = Outputs(rx, A, S, N)

    def run(case, iters=2):
        xs = rows.build(case, A, S, N)
        ins = [rx.alloc(x.nbytes).upload(x) for x in xs]
        out.refill()
        rx.precombine_dev([b.ptr for b in ins], S, N, out.dev["y"].ptr, iters, out.dev["w"].ptr, out.dev["s"].ptr)
        rx.sync()
        for b in ins:
            b.free()
        return xs, out.split(out.download(), N)[0]
    try:
        for case, bad in (("zero_slot", [0]), ("nan_first", [0]), ("nan_later", [0]), ("inf", [0, N - 1])):
            xs, (y, w, s) = run(case)
            deg = np.flatnonzero(s["flags"])
            assert list(deg) == bad and rows.same_bits(y[deg], xs[0][deg]) and (w[deg, 0] == 1).all() and (w[deg, 1:] == 0).all()
        xs, (y, w, s) = run("tie", 0)
        assert (s["ref"] == 1).all() and not s["flags"].any()
        xs, (y, w, s) = run("known_gain")
        want, r = rows.known_gain_weights(A)
        assert (s["ref"] == r).all() and np.allclose(w, want, atol=1e-5) and (w[:, r].imag == 0).all()
        xs, (y, w, s) = run("zero_antenna")
        assert (w[:, 1] == 0).all()
    finally:
        out.free()


def test_weights_and_stats_are_optional(rx):
    A, S = 3, 320
    xs = rows.build("scene", A, S, N, seed=2)
    ins = [rx.alloc(x.nbytes).upload(x) for x in xs]
    out = Outputs(rx, A, S, N)
    want = pr.combine(xs, S, 2)
    try:
        for with_w in (False, True):
            for with_s in (False, True):
                out.refill()
                rx.precombine_dev([b.ptr for b in ins], S, N, out.dev["y"].ptr, 2, out.dev["w"].ptr if with_w else None,
                                  out.dev["s"].ptr if with_s else None)
                rx.sync()
                raw = out.download()
                (y, w, s), clean = out.split(raw, N)
                assert clean and rows.same_bits(y, want[0])
                assert rows.same_bits(w, want[1]) if with_w else out.untouched(raw, ("w",))
                assert rows.same_bits(s, want[2]) if with_s else out.untouched(raw, ("s",))
    finally:
        out.free()
        for b in ins:
            b.free()


# ---- in front of the demod -----------------------------------------------------------------------------------------------------

def two_antenna_batch(rx, n=64, plen=40, snr_db=14.0):
    """n frames over the eight rates through two flat channels of independent noise, on the device: (DevBufs, slot, psdus)"""
    enc = (np.arange(n) % 8).astype(np.uint8)
    slot = (160 + txgen.frame_samples(plen, 0) + 79 + 63) // 64 * 64
    psdus = txgen.make_psdus(n, plen, seed=5)
    tx = rx.alloc(n * slot * 8)
    iqs = [rx.alloc(n * slot * 8) for _ in range(2)]
    rx.tx_batch_dev(tx.ptr, n * slot, psdus, enc, lead=160, row_len=slot)
    for a, iq in enumerate(iqs):
        rx.channel_dev(tx.ptr, iq.ptr, n * slot, n, row_len=slot, taps=(np.exp(1j * (0.4 + 2.1 * a)),), gain=math.sqrt(10 ** (snr_db / 10)),
                       noise_voltage=1.0, seed=300 + a)
    rx.sync()
    tx.free()
    return iqs, slot, psdus


@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
def test_queued_without_a_sync_gives_the_synchronised_bytes(rx, soft):
    n = 64
    iqs, slot, psdus = two_antenna_batch(rx)
    got = []
    try:
        for synced in (False, True):
            step = rx.sync if synced else (lambda: None)
            y, w = rx.alloc(n * slot * 8), rx.alloc(n * 2 * 8)
            out = rx.alloc_out(n, psdu_stride=64)
            try:
                rx.precombine_dev([b.ptr for b in iqs], slot, n, y.ptr, 2, w.ptr)
                step()
                rx.demod_batch_dev(y.ptr, slot, n, out)
                step()
                (rx.decode_batch_soft_dev if soft else rx.decode_batch_dev)(n, out)
                rx.sync()
                r = rx.download_out(out, n)
                r["weights"], r["y"] = w.download(np.complex64, n * 2), y.download(np.complex64, n * slot)
                got.append(r)
            finally:
                rx.free_out(out)
                y.free()
                w.free()
        a, b = got
        for k in ("frames", "idx", "llr", "carrier", "psdu", "weights", "y"):
            assert rows.same_bits(a[k], b[k]), k
        ok = (a["frames"]["flags"] & capi.F_CRC_OK) != 0
        assert ok.sum() >= n // 4 and np.array_equal(a["psdu"][ok][:, :40], psdus[ok])
    finally:
        for b in iqs:
            b.free()


def test_host_conveniences(rx):
    """WifiRx.precombine and WifiRx.demod_precombined on host arrays: the reference's row set, and the frames of demodulating it"""
    n, plen = 16, 40
    iqs, slot, psdus = two_antenna_batch(rx, n=n, snr_db=28.0)
    xs = [b.download(np.complex64, n * slot) for b in iqs]
    for b in iqs:
        b.free()
    y, w, s = rx.precombine(xs, slot, iters=1)
    want = pr.combine(xs, slot, 1)
    assert rows.same_bits(y, want[0]) and rows.same_bits(w, want[1]) and rows.same_bits(s, want[2])
    for soft in (False, True):
        r = rx.demod_precombined(xs, slot, iters=1, soft=soft, psdu_stride=64)
        assert ((r["frames"]["flags"] & capi.F_CRC_OK) != 0).all() and np.array_equal(r["psdu"][:, :plen], psdus), soft
        assert rows.same_bits(r["weights"], w) and rows.same_bits(r["pre_stats"], s)
        one = rx.demod_batch(y.reshape(-1), slot, decode=True, psdu_stride=64, soft=soft)
        assert np.array_equal(r["frames"], one["frames"]) and np.array_equal(r["psdu"], one["psdu"]) and rows.same_bits(r["carrier"], one["carrier"])
    with pytest.raises(ValueError):
        rx.demod_precombined([xs[0], xs[1][:-1]], slot)
    with pytest.raises(ValueError):
        rx.precombine([], slot)


# ---- what it is for ------------------------------------------------------------------------------------------------------------

def lost_frames(point, want_mrc):
    """the scene of tests/precombine_point.py on the device, hard decode_mac: lost frames of each antenna alone, of rule 33
    with ONE demod and, on request, of rule 23's MRC over the A demods; and the CRC_OK frames with a wrong PSDU"""
    A, snr_db = point["n_ant"], point["snr_db"]
    n, enc, plen = pt.N, pt.ENC, pt.PLEN
    n_sym, slot = pt.geometry()
    stride = 112
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=2, want_carrier=True, device=0)
    bufs, outs = [], []
    try:
        psdus = txgen.make_psdus(n, plen, seed=pt.PSDU_SEED)
        d_psdu = rx.alloc(n * plen).upload(psdus)
        tx, y = rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
        iqs = [rx.alloc(n * slot * 8) for _ in range(A)]
        bufs += [tx, y] + iqs
        rx.tx_batch_dev(tx.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=pt.LEAD, row_len=slot)
        ref = rx.alloc_out(n)
        outs.append(ref)
        rx.demod_batch_dev(tx.ptr, slot, n, ref)
        ref["psdu"], ref["psdu_stride"] = d_psdu, plen
        assert rx.link_stats(n, ref, ref)["frames_ref"] == n
        lost, wrong = {"single": []}, 0

        def score(dev):
            nonlocal wrong
            rx.decode_batch_dev(n, dev)
            r = rx.link_stats(n, dev, ref)
            wrong += r["frames_crc_ok_wrong"]
            return r["frames_ref"] - r["frames_psdu_ok"]

        for a, (seed, fade_seed) in enumerate(pt.SEEDS[:A]):
            rx.channel_dev(tx.ptr, iqs[a].ptr, n * slot, n, row_len=slot, gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=seed,
                           doppler=0.0, fade_seed=fade_seed)
            outs.append(rx.alloc_out(n, psdu_stride=stride, want_csi=True))
            rx.demod_batch_dev(iqs[a].ptr, slot, n, outs[-1])
            lost["single"].append(score(outs[-1]))
        out = rx.alloc_out(n, psdu_stride=stride)
        outs.append(out)
        if want_mrc:
            rx.diversity_combine_dev(outs[1:1 + A], n, out, capi.DIV_MRC)
            lost["mrc"] = score(out)
        rx.precombine_dev([b.ptr for b in iqs], slot, n, y.ptr, pt.ITERS)
        rx.demod_batch_dev(y.ptr, slot, n, out)
        lost["precombine"] = score(out)
        lost["crc_ok_wrong"] = wrong
        return lost
    finally:
        for d in outs:
            rx.free_out(d)
        for b in bufs:
            b.free()
        rx.close()


def test_gain_at_two_antennas():
    """2048 QPSK-1/2 frames of 100 bytes, flat Rayleigh, two antennas at 12 dB (tests/precombine_point.py, point a2; the host
    chain in the rule's own arithmetic lost 56 against 424 and 428 of 2048: profiles/precombine_operating_point.json).
    Asserted: pre-detection combining with one demod loses at most half of what the better single antenna loses."""
    lost = lost_frames(pt.POINTS["a2"], False)
    print("lost frames of %d:" % pt.N, lost)
    assert lost["crc_ok_wrong"] == 0
    assert 2 * lost["precombine"] <= min(lost["single"]), lost


def test_gain_at_four_antennas():
    """the same scene with four antennas at 8 dB (point a4; the host chain lost 8 against rule 23's 46 and 883 .. 913 alone).
    Asserted: pre-detection combining with one demod loses no more frames than rule 23's MRC over four demods."""
    lost = lost_frames(pt.POINTS["a4"], True)
    print("lost frames of %d:" % pt.N, lost)
    assert lost["crc_ok_wrong"] == 0
    assert lost["precombine"] <= lost["mrc"], lost


# ---- refused arguments ---------------------------------------------------------------------------------------------------------

def _refusals():
    """(name, expected code, how the good call is bent): a(rgs) has n_ant, ptrs (list), slot_len, n_slots, iters, out, w, s"""
    E, R = capi.EINVAL, capi.ERANGE

    def key(name, value):
        def bend(a):
            a[name] = value(a[name]) if callable(value) else value
        return bend

    def ptr(i, value):
        def bend(a):
            a["ptrs"][i] = value(a["ptrs"][i]) if callable(value) else value
        return bend

    def alias(i):
        def bend(a):
            a["out"] = a["ptrs"][i]
        return bend
    return [
        ("null iq_dev", E, key("ptrs", None)), ("null antenna 0", E, ptr(0, None)), ("null antenna 1", E, ptr(1, None)), ("null out", E, key("out", None)),
        ("n_ant 0", E, key("n_ant", 0)), ("n_ant 9", E, key("n_ant", 9)),
        ("slot_len 0", E, key("slot_len", 0)), ("slot_len 32", E, key("slot_len", 32)), ("slot_len 96", E, key("slot_len", 96)),
        ("slot_len 65600", E, key("slot_len", 65600)), ("iters 5", E, key("iters", 5)),
        ("misaligned antenna 0", E, ptr(0, lambda p: p + 4)), ("misaligned antenna 1", E, ptr(1, lambda p: p + 4)),
        ("misaligned out", E, key("out", lambda p: p + 4)), ("misaligned weights", E, key("w", lambda p: p + 4)),
        ("misaligned stats", E, key("s", lambda p: p + 4)),
        ("out is antenna 0", E, alias(0)), ("out is antenna 1", E, alias(1)),
        ("too many slots", R, key("n_slots", 65)),
    ]


@pytest.mark.parametrize("name,code,bend", _refusals(), ids=[r[0] for r in _refusals()])
def test_refused_arguments_queue_nothing(rx, name, code, bend):
    A, S, n = 2, 64, 4
    xs = rows.build("scene", A, S, 65)
    ins = [rx.alloc(x.nbytes).upload(x) for x in xs]
    out = Outputs(rx, A, S, 65)
    try:
        a = dict(n_ant=A, ptrs=[b.ptr for b in ins], slot_len=S, n_slots=n, iters=2, out=out.dev["y"].ptr, w=out.dev["w"].ptr, s=out.dev["s"].ptr)
        bend(a)
        arr = None if a["ptrs"] is None else (C.c_void_p * 8)(*a["ptrs"])
        rc = capi.lib().wifirx_precombine(rx._h, a["n_ant"], arr, a["slot_len"], a["n_slots"], a["iters"], a["out"], a["w"], a["s"])
        assert rc == code, (name, rc, capi.lib().wifirx_last_error(rx._h))
        assert capi.lib().wifirx_last_error(rx._h) != b""
        rx.sync()
        assert out.untouched(out.download()), name
        assert all(np.array_equal(b.download(np.complex64, x.size), x.reshape(-1)) for b, x in zip(ins, xs))
    finally:
        out.free()
        for b in ins:
            b.free()


def test_no_slots_is_ok_and_does_nothing(rx):
    xs = rows.build("scene", 2, 64, 1)
    ins = [rx.alloc(x.nbytes).upload(x) for x in xs]
    out = Outputs(rx, 2, 64, 1)
    try:
        rx.precombine_dev([b.ptr for b in ins], 64, 0, out.dev["y"].ptr, 2, out.dev["w"].ptr, out.dev["s"].ptr)
        rx.sync()
        assert out.untouched(out.download())
    finally:
        out.free()
        for b in ins:
            b.free()
