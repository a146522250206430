"""wifirx_diversity_combine (wr_diversity.hip) on the device: bit for bit against tests/diversity_ref.py on the host-built rows
of tests/diversity_rows.py (every clause of NUMERICS.md rule 23, outputs between sentinels), its identity with the demod for
one antenna and for the same batch twice, its place on the stream, the refused arguments, and what it is for: fewer lost
frames behind two antennas in Rayleigh fading."""
import ctypes as C
import math

import numpy as np
import pytest

import diversity_point as pt
import diversity_ref as dr
import diversity_rows as rows
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

FILL = 0xA5
N, MS = rows.N_SLOTS, rows.MAX_SYM


@pytest.fixture(scope="module")
def handles():
    """llr_bits 6, 2 and 0 at the geometry of the rows; max_batch 64 for the range check"""
    h = {b: capi.WifiRx(max_sym=MS, llr_bits=b, want_carrier=True, max_batch=64, device=0) for b in (6, 2, 0)}
    yield h
    for r in h.values():
        r.close()


def upload_inputs(rx, frames, carrier, csi):
    ins = [dict(frames=rx.alloc(f.nbytes).upload(f), carrier=rx.alloc(c.nbytes).upload(c), csi=rx.alloc(h.nbytes).upload(h))
           for f, c, h in zip(frames, carrier, csi)]
    return ins


def free_all(dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, capi.DevBuf):
                v.free()


def sentinel_outputs(rx, host):
    """device buffers holding the sentinel arrays of dr.new_outputs()"""
    return {k: rx.alloc(v.nbytes).upload(v) for k, v in host.items() if v is not None}


def refill(dev, host):
    for k, v in host.items():
        if v is not None:
            dev[k].upload(v)


def download(dev, host):
    return {k: (dev[k].download(v.dtype, v.size).reshape(v.shape) if v is not None else None) for k, v in host.items()}


@pytest.mark.parametrize("case", rows.CASES)
@pytest.mark.parametrize("n_ant", rows.N_ANT)
def test_rows_equal_the_reference(handles, n_ant, case):
    frames, carrier, csi = rows.build(case, n_ant)
    ins = upload_inputs(handles[6], frames, carrier, csi)
    g = rows.gains(n_ant)
    try:
        for bits in (6, 2):
            rx = handles[bits]
            for bf in (False, True):
                rx.set_llr_format("bf16" if bf else "f32")
                fresh = dr.new_outputs(N, MS, bits, bf16=bf, fill=FILL)
                dev = sentinel_outputs(rx, fresh)
                try:
                    for csi_on in (0, 1):
                        rx.set_param(capi.P_LLR_CSI, csi_on)
                        for mode in (capi.DIV_MRC, capi.DIV_SELECT):
                            for gain in (None, g):
                                refill(dev, fresh)
                                rx.diversity_combine_dev(ins, N, dev, mode, gain, dev["used_mask"].ptr)
                                rx.sync()
                                got = download(dev, fresh)
                                want = dr.combine(frames, carrier, csi, MS, bits, dr.new_outputs(N, MS, bits, bf16=bf, fill=FILL), mode=mode,
                                                  ant_gain=gain, llr_csi=bool(csi_on), bf16=bf)
                                bad = rows.same_outputs(got, want, bf)
                                assert not bad, (bits, bf, csi_on, mode, gain is not None, bad)
                finally:
                    free_all([dev])
                    rx.set_llr_format("f32")
                    rx.set_param(capi.P_LLR_CSI, 0)
    finally:
        free_all(ins)


def test_optional_outputs_and_more_slots_than_the_grid_has_waves(handles):
    """every subset of idx / llr / carrier / used_mask, and a batch of 64 slots on a handle whose other outputs are absent"""
    rx = handles[6]
    frames, carrier, csi = rows.build("other_psdu_len", 3, seed=5, n_slots=64)
    ins = upload_inputs(rx, frames, carrier, csi)
    fresh = dr.new_outputs(64, MS, 6, fill=FILL)
    dev = sentinel_outputs(rx, fresh)
    try:
        for keep in (("idx",), ("llr",), ("carrier",), (), ("idx", "llr", "carrier")):
            refill(dev, fresh)
            part = {k: v for k, v in dev.items() if k in keep or k == "frames"}
            mask = dev["used_mask"].ptr if keep else None
            rx.diversity_combine_dev(ins, 64, part, capi.DIV_MRC, None, mask)
            rx.sync()
            got = download(dev, fresh)
            want = dr.new_outputs(64, MS, 6, fill=FILL)
            for k in ("idx", "llr", "carrier", "used_mask"):
                if not (k in keep or (k == "used_mask" and keep)):
                    want[k] = None
            dr.combine(frames, carrier, csi, MS, 6, want)
            for k, v in fresh.items():              # what was not asked for still holds the sentinel
                if want.get(k) is None:
                    want[k] = v
            assert not rows.same_outputs(got, want, False), keep
    finally:
        free_all(ins + [dev])


# ---- identity with the demod ---------------------------------------------------------------------------------------------------

def demodulated_batch(rx, n=64, plen=40, snr_db=25.0):
    """n frames over the eight rates through an AWGN channel, on the device: (iq DevBuf, slot, n_sym of the longest)"""
    enc = (np.arange(n) % 8).astype(np.uint8)
    slot = 160 + txgen.frame_samples(plen, 0) + 79
    slot += slot & 1
    psdus = txgen.make_psdus(n, plen, seed=5)
    tx, iq = rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
    rx.tx_batch_dev(tx.ptr, n * slot, psdus, enc, lead=160, row_len=slot)
    rx.channel_dev(tx.ptr, iq.ptr, n * slot, n, row_len=slot, gain=math.sqrt(10 ** (snr_db / 10)), noise_voltage=1.0, seed=77)
    rx.sync()
    tx.free()
    return iq, slot, psdus


@pytest.fixture(scope="module")
def rx15():
    r = capi.WifiRx(max_sym=txgen.n_sym_for(40, 0), llr_bits=6, want_carrier=True, device=0)
    yield r
    r.close()


@pytest.mark.parametrize("bf", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("csi_on", (0, 1))
def test_one_antenna_returns_the_demod_s_outputs_and_two_copies_double_the_llrs(rx15, csi_on, bf):
    rx, n, ms = rx15, 64, rx15.max_sym
    iq, slot, _ = demodulated_batch(rx)
    rx.set_llr_format("bf16" if bf else "f32")
    rx.set_param(capi.P_LLR_CSI, csi_on)
    src = rx.alloc_out(n, want_csi=True)
    fresh = dr.new_outputs(n, ms, 6, bf16=bf, fill=FILL)
    dev = sentinel_outputs(rx, fresh)
    try:
        rx.demod_batch_dev(iq.ptr, slot, n, src)
        rx.diversity_combine_dev([src], n, dev, capi.DIV_MRC, None, dev["used_mask"].ptr)       # no sync in between
        rx.sync()
        d, one = rx.download_out(src, n), download(dev, fresh)
        fr = d["frames"]
        assert ((fr["flags"] & rows.GOOD) == rows.GOOD).all() and set(fr["encoding"]) == set(range(8))
        assert np.array_equal(one["frames"], fr) and (one["used_mask"] == 1).all()
        for i in range(n):
            ns, nb = int(fr["n_sym"][i]), int(fr["n_bpsc"][i])
            assert np.array_equal(one["idx"][i, :ns], d["idx"][i, :ns]) and (one["idx"][i, ns:] == FILL).all()
            assert rows.same_bits(one["carrier"][i, :ns], d["carrier"][i, :ns])
            assert np.array_equal(one["llr"][i, :ns * 48 * nb], d["llr"][i, :ns * 48 * nb])
            assert rows.same_bits(one["llr"][i, ns * 48 * nb:], fresh["llr"][i, ns * 48 * nb:])
        # the same batch as two antennas
        refill(dev, fresh)
        rx.diversity_combine_dev([src, src], n, dev, capi.DIV_MRC, None, dev["used_mask"].ptr)
        rx.sync()
        two = download(dev, fresh)
        assert (two["used_mask"] == 3).all() and np.array_equal(two["frames"], fr)
        assert rows.same_bits(two["carrier"], one["carrier"]) and np.array_equal(two["idx"], one["idx"])
        wide = (lambda v: capi.bf16_to_f32(v)) if bf else (lambda v: v)
        for i in range(n):
            nv = int(fr["n_sym"][i]) * 48 * int(fr["n_bpsc"][i])
            a, b = wide(two["llr"][i, :nv]), wide(one["llr"][i, :nv])
            assert np.array_equal(a, np.float32(2) * b if csi_on else b), i
    finally:
        rx.set_llr_format("f32")
        rx.set_param(capi.P_LLR_CSI, 0)
        rx.free_out(src)
        free_all([dev])
        iq.free()


@pytest.mark.parametrize("soft", (False, True), ids=("hard", "soft"))
def test_queued_without_a_sync_gives_the_synchronised_bytes(rx15, soft):
    rx, n = rx15, 64
    iq, slot, psdus = demodulated_batch(rx, snr_db=14.0)
    got = []
    try:
        for synced in (False, True):
            step = rx.sync if synced else (lambda: None)
            ins = [rx.alloc_out(n, want_csi=True) for _ in range(2)]
            out = rx.alloc_out(n, psdu_stride=64)
            mask = rx.alloc(n).upload(np.zeros(n, np.uint8))
            try:
                for d in ins:
                    rx.demod_batch_dev(iq.ptr, slot, n, d)
                    step()
                rx.diversity_combine_dev(ins, n, out, capi.DIV_MRC, [1.0, 0.5], mask.ptr)
                step()
                (rx.decode_batch_soft_dev if soft else rx.decode_batch_dev)(n, out)
                rx.sync()
                r = rx.download_out(out, n)
                r["used_mask"] = mask.download(np.uint8, n)
                got.append(r)
            finally:
                for d in ins + [out]:
                    rx.free_out(d)
                mask.free()
        a, b = got
        for k in ("frames", "idx", "llr", "carrier", "psdu", "used_mask"):
            assert rows.same_bits(a[k], b[k]), k
        ok = (a["frames"]["flags"] & capi.F_CRC_OK) != 0
        assert ok.sum() >= n // 4 and np.array_equal(a["psdu"][ok][:, :40], psdus[ok])
    finally:
        iq.free()


def test_host_convenience_demodulates_combines_and_decodes(rx15):
    """WifiRx.demod_diversity on host arrays: two antennas behind independent noise, every rate; the PSDUs are the transmitted
    ones, both antennas contribute, and the combined points are the reference's of the two single-antenna demods"""
    rx, n, plen, ms = rx15, 16, 40, rx15.max_sym
    enc = (np.arange(n) % 8).astype(np.uint8)
    slot = 160 + txgen.frame_samples(plen, 0) + 79
    slot += slot & 1
    psdus = txgen.make_psdus(n, plen, seed=6)
    tx = rx.tx_batch(psdus, enc, lead=160, row_len=slot)
    iqs = [rx.channel(tx, gain=math.sqrt(10 ** 2.8), noise_voltage=1.0, seed=500 + a) for a in range(2)]
    singles = []
    for x in iqs:
        dev = rx.alloc_out(n, want_csi=True)
        d_iq = rx.alloc(x.nbytes).upload(x)
        rx.demod_batch_dev(d_iq.ptr, slot, n, dev)
        rx.sync()
        singles.append(rx.download_out(dev, n))
        rx.free_out(dev)
        d_iq.free()
    for soft in (False, True):
        for mode in ("mrc", "select"):
            r = rx.demod_diversity(iqs, slot, mode=mode, soft=soft, psdu_stride=64)
            assert ((r["frames"]["flags"] & capi.F_CRC_OK) != 0).all() and np.array_equal(r["psdu"][:, :plen], psdus), (soft, mode)
            want = dr.new_outputs(n, ms, 6, fill=0)
            dr.combine([s["frames"] for s in singles], [s["carrier"] for s in singles], [s["csi"] for s in singles], ms, 6, want,
                       mode=dr.MRC if mode == "mrc" else dr.SELECT)
            assert np.array_equal(r["used_mask"], want["used_mask"]) and ((r["used_mask"] == 3).all() if mode == "mrc" else True)
            assert rows.same_bits(r["carrier"], want["carrier"]) and np.array_equal(r["idx"], want["idx"]) and rows.same_bits(r["llr"], want["llr"])
    with pytest.raises(ValueError):
        rx.demod_diversity([iqs[0], iqs[1][:-1]], slot)


# ---- what it is for ----------------------------------------------------------------------------------------------------------

def test_diversity_gain():
    """2048 QPSK-1/2 frames of 100 bytes, flat Rayleigh with one static gain per row and antenna, two antennas at the mean SNR
    of tests/diversity_point.py (chosen on the host chain: profiles/diversity_operating_point.json; single-antenna FER 0.21).
    Asserted, for the hard and for the soft decoder: every CRC_OK PSDU is the transmitted one; lost frames MRC < SELECT < the
    better single antenna; MRC loses at most half of what the better single antenna loses (outage theory: a seventh,
    1 - e^-x (1 + x) against 1 - e^-x at x = 0.28; the factor 2 is the margin for 2048 frames and for detection losses)."""
    n, enc, plen = pt.N, pt.ENC, pt.PLEN
    n_sym, slot = pt.geometry()
    stride = 112
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=2, want_carrier=True, device=0)
    bufs = []
    try:
        psdus = txgen.make_psdus(n, plen, seed=pt.PSDU_SEED)
        d_psdu = rx.alloc(n * plen).upload(psdus)
        tx, iq = rx.alloc(n * slot * 8), rx.alloc(n * slot * 8)
        bufs += [tx, iq]
        rx.tx_batch_dev(tx.ptr, n * slot, d_psdu.ptr, enc, psdu_len=np.full(n, plen, np.uint32), psdu_stride=plen, lead=pt.LEAD, row_len=slot)
        ref = rx.alloc_out(n)
        rx.demod_batch_dev(tx.ptr, slot, n, ref)
        ref["psdu"], ref["psdu_stride"] = d_psdu, plen
        assert rx.link_stats(n, ref, ref)["frames_ref"] == n
        ins, lost, wrong = [], {}, 0

        def score(dev, name):
            nonlocal wrong
            for soft in (False, True):
                (rx.decode_batch_soft_dev if soft else rx.decode_batch_dev)(n, dev)
                r = rx.link_stats(n, dev, ref)
                lost[name, soft] = r["frames_ref"] - r["frames_psdu_ok"]
                wrong += r["frames_crc_ok_wrong"]

        for a, (seed, fade_seed) in enumerate(pt.SEEDS):
            rx.channel_dev(tx.ptr, iq.ptr, n * slot, n, row_len=slot, gain=math.sqrt(10 ** (pt.SNR_DB / 10)), noise_voltage=1.0, seed=seed,
                           doppler=0.0, fade_seed=fade_seed)
            ins.append(rx.alloc_out(n, psdu_stride=stride, want_csi=True))
            rx.demod_batch_dev(iq.ptr, slot, n, ins[a])
            score(ins[a], "ant%d" % a)
        out = rx.alloc_out(n, psdu_stride=stride)
        for name, mode in (("select", capi.DIV_SELECT), ("mrc", capi.DIV_MRC)):
            rx.diversity_combine_dev(ins, n, out, mode)
            score(out, name)
        print("lost frames of %d (hard, soft):" % n, {k: (lost[k, False], lost[k, True]) for k in ("ant0", "ant1", "select", "mrc")})
        assert wrong == 0
        for soft in (False, True):
            single = min(lost["ant0", soft], lost["ant1", soft])
            assert 0.1 * n <= single <= 0.5 * n, (soft, single)
            assert lost["mrc", soft] < lost["select", soft] < single, (soft, lost)
            assert 2 * lost["mrc", soft] <= single, (soft, lost)
        for d in ins + [out]:
            rx.free_out(d)
        rx.free_out(ref)
    finally:
        for b in bufs:
            b.free()
        rx.close()


# ---- refused arguments ---------------------------------------------------------------------------------------------------------

def _refusals():
    """(name, expected code, how the good call is bent): a(rgs) has n_ant, ins (list of Out), n_slots, mode, gain, out, mask"""
    E, R = capi.EINVAL, capi.ERANGE

    def field(which, name, value):
        def bend(a):
            o = a["out"] if which == "out" else a["ins"][which]
            setattr(o, name, value(getattr(o, name)) if callable(value) else value)
        return bend

    def gain(v):
        def bend(a):
            a["gain"] = [1.0, v]
        return bend

    def key(name, value):
        def bend(a):
            a[name] = value
        return bend

    def alias(name):
        def bend(a):
            setattr(a["out"], name, getattr(a["ins"][1], name))
        return bend
    return [
        ("null in", E, key("ins", None)), ("null out", E, key("out", None)), ("null out frames", E, field("out", "frames", None)),
        ("n_ant 0", E, key("n_ant", 0)), ("n_ant 9", E, key("n_ant", 9)), ("unknown mode", E, key("mode", 2)), ("negative mode", E, key("mode", -1)),
        ("host input", E, field(1, "on_device", 0)), ("host output", E, field("out", "on_device", 0)),
        ("misaligned input carrier", E, field(0, "carrier", lambda p: p + 8)), ("misaligned input csi", E, field(1, "csi", lambda p: p + 8)),
        ("misaligned input frames", E, field(1, "frames", lambda p: p + 4)), ("misaligned output idx", E, field("out", "idx", lambda p: p + 4)),
        ("misaligned output llr", E, field("out", "llr", lambda p: p + 8)), ("misaligned output carrier", E, field("out", "carrier", lambda p: p + 8)),
        ("misaligned output frames", E, field("out", "frames", lambda p: p + 8)),
        ("no frames", E, field(1, "frames", None)), ("no carrier", E, field(0, "carrier", None)), ("no csi", E, field(1, "csi", None)),
        ("gain nan", E, gain(float("nan"))), ("gain inf", E, gain(float("inf"))), ("gain negative", E, gain(-0.5)),
        ("hbits given", E, field("out", "hbits", lambda p: 4096)),
        ("output frames are an input's", E, alias("frames")), ("output carrier is an input's", E, alias("carrier")),
        ("too many slots", R, key("n_slots", 65)),
    ]


@pytest.mark.parametrize("name,code,bend", _refusals(), ids=[r[0] for r in _refusals()])
def test_refused_arguments_queue_nothing(handles, name, code, bend):
    rx = handles[6]
    frames, carrier, csi = rows.build("all_usable", 2, n_slots=64)
    ins = upload_inputs(rx, frames, carrier, csi)
    fresh = dr.new_outputs(64, MS, 6, fill=FILL)
    dev = sentinel_outputs(rx, fresh)
    try:
        a = dict(n_ant=2, ins=[rx._out_struct(d) for d in ins], n_slots=N, mode=capi.DIV_MRC, gain=None, out=rx._out_struct(dev),
                 mask=dev["used_mask"].ptr)
        bend(a)
        arr = None if a["ins"] is None else (capi.Out * 2)(*a["ins"])
        g = None if a["gain"] is None else (C.c_float * 2)(*a["gain"])
        out = None if a["out"] is None else C.byref(a["out"])
        rc = capi.lib().wifirx_diversity_combine(rx._h, a["n_ant"], arr, a["n_slots"], a["mode"], g, out, a["mask"])
        assert rc == code, (name, rc, capi.lib().wifirx_last_error(rx._h))
        assert capi.lib().wifirx_last_error(rx._h) != b""
        rx.sync()
        got = download(dev, fresh)
        assert not rows.same_outputs(got, fresh, False), name
    finally:
        free_all(ins + [dev])


def test_llr_on_a_handle_without_llrs_is_refused_and_no_slots_is_ok(handles):
    rx0, rx6 = handles[0], handles[6]
    frames, carrier, csi = rows.build("all_usable", 2)
    ins = upload_inputs(rx6, frames, carrier, csi)
    fresh = dr.new_outputs(N, MS, 6, fill=FILL)
    dev = sentinel_outputs(rx6, fresh)
    try:
        with pytest.raises(capi.WifiRxError) as e:
            rx0.diversity_combine_dev(ins, N, dev)
        assert e.value.code == capi.EINVAL
        part = {k: v for k, v in dev.items() if k != "llr"}
        rx6.diversity_combine_dev(ins, 0, dev, capi.DIV_MRC, None, dev["used_mask"].ptr)           # n_slots = 0: OK, nothing happens
        rx0.sync(), rx6.sync()
        assert not rows.same_outputs(download(dev, fresh), fresh, False)
        rx0.diversity_combine_dev(ins, N, part, capi.DIV_SELECT)                                   # without llr the handle combines
        rx0.sync()
        want = dr.new_outputs(N, MS, 0, fill=FILL)
        want["llr"] = None
        dr.combine(frames, carrier, csi, MS, 0, want, mode=dr.SELECT)
        want["llr"], want["used_mask"] = fresh["llr"], fresh["used_mask"]
        assert not rows.same_outputs(download(dev, fresh), want, False)
    finally:
        free_all(ins + [dev])
