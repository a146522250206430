"""wifirx_channel, the device channel_model (wr_channel.hip), through the C ABI and the block:
  * bit for bit NUMERICS.md rule 17 (tests/channel_ref.py) on the noiseless path: 1, 2, 8 and 64 taps, fixed rows and row_off
    rows (lengths 0, 1, odd), host and device taps, both pair alignments of the output; every row sample written, nothing else;
  * the noise: wifirx_synth_slots' bit for bit on zero input, the restatement's to 1e-5, and continued by sample0;
  * in place with one tap; argument errors refused on the host, before any launch;
  * config 3 through TX -> channel -> demod -> decode_mac on the device against the CPU oracle's table;
  * IRS_tranceiver's loop-back through wifi_phy_tx -> x gain -> channel_model -> wifi_phy_rx."""
import math
import os

import numpy as np
import pytest

import channel_ref
from channel_helpers import NAN_WORD, P, assert_oracle_records, cnoise, loopback, run, rx, tap_sets  # noqa: F401 (rx: fixture)
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFO_20PPM = 2 * np.pi * 20e-6 * 5.89e9 / 20e6


@pytest.mark.parametrize("L", [1, 2, 8, 64])
def test_noiseless_bit_exact_fixed_rows(rx, L):
    rng = np.random.default_rng(L)
    for row_len, n_rows in ((4608, 5), (1472, 7), (1001, 4), (3, 9)):
        x = cnoise(rng, row_len * n_rows)
        taps = tap_sets(rng, 3, L)
        cfo = rng.uniform(-0.05, 0.05, n_rows).astype(np.float32)
        want = channel_ref.channel(x.reshape(n_rows, row_len), taps=taps, cfo=cfo, phase0=0x123456789ABCDEF, gain=1.7)
        for shift in (0, 1):
            for dev in (False, True):
                got = run(rx, x, x.size, n_rows, shift, taps=taps, taps_dev=dev, row_len=row_len, cfo=cfo,
                          phase0=0x123456789ABCDEF, gain=1.7)
                assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)), (L, row_len, shift, dev)


@pytest.mark.parametrize("L", [1, 2, 8, 64])
def test_noiseless_bit_exact_row_off(rx, L):
    """rows of 0, 1, odd and long lengths, starting 5 samples into the buffer and ending 7 before its end: the samples
    outside the rows keep their NaN pattern"""
    rng = np.random.default_rng(100 + L)
    lens = [0, 1, 2, 7, 0, 2049, 4096, 1, 63, 64, 65, 5000, 0, 3]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(5)
    cap = int(off[-1]) + 7
    x = cnoise(rng, cap)
    taps = tap_sets(rng, 5, L)
    cfo = rng.uniform(-0.05, 0.05, len(lens)).astype(np.float32)
    want = channel_ref.channel(x, row_off=off, taps=taps, cfo=cfo, gain=0.5)
    inside = np.zeros(cap, bool)
    inside[int(off[0]):int(off[-1])] = True
    for shift in (0, 1):
        for dev in (False, True):
            got = run(rx, x, cap, len(lens), shift, taps=taps, taps_dev=dev, row_off=off, cfo=cfo, gain=0.5)
            assert np.array_equal(got[inside].view(np.uint32), want[inside].view(np.uint32)), (L, shift, dev)
            assert (got[~inside].view(np.uint32) == NAN_WORD).all(), (L, shift, dev)


def test_zero_input_is_synth_slots_noise(rx):
    slot, n_slots, seed = 4608, 64, 0xDEADBEEF12345
    slots = rx.alloc(slot * n_slots * 8)
    rx.synth_slots(np.zeros((1, 100), np.complex64), slots.ptr, slot, n_slots, 160, 20.0, 0.03, seed)
    want = slots.download(np.complex64, slot * n_slots)
    slots.free()
    got = run(rx, np.zeros(slot * n_slots, np.complex64), slot * n_slots, n_slots, row_len=slot, gain=1.0,
              noise_voltage=1.0, seed=seed)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_noise_against_the_restatement(rx):
    rng = np.random.default_rng(7)
    off = np.array([0, 1000, 1001, 3500, 3503, 8000], np.uint64)
    x = cnoise(rng, 8000)
    taps = tap_sets(rng, 2, 8)
    cfo = rng.uniform(-0.05, 0.05, 5).astype(np.float32)
    kw = dict(row_off=off, taps=taps, cfo=cfo, phase0=77, gain=2.0, noise_voltage=0.3, seed=99, sample0=12345)
    want = channel_ref.channel(x, **kw)
    got = run(rx, x, 8000, 5, **kw)
    assert np.abs(got - want).max() <= 1e-5
    # and the noise itself: variance noise_voltage^2, split evenly
    z = run(rx, np.zeros(1 << 20, np.complex64), 1 << 20, 1, row_len=1 << 20, noise_voltage=0.3, seed=5).astype(np.complex128)
    assert abs(np.mean(np.abs(z) ** 2) / 0.09 - 1) < 0.01
    assert abs(np.var(z.real) / np.var(z.imag) - 1) < 0.01


@pytest.mark.parametrize("k", [1, 2, 777, 4096])
def test_sample0_continues_the_one_shot_call(rx, k):
    rng = np.random.default_rng(k)
    n = 9000
    x = cnoise(rng, n)
    cfo = np.float32(0.021)
    inc = capi.phase_inc(cfo)
    kw = dict(taps=[0.8 - 0.1j], cfo=cfo, gain=1.5, noise_voltage=0.7, seed=321)
    one = run(rx, x, n, 1, row_len=n, **kw)
    part = run(rx, x[k:], n - k, 1, row_len=n - k, phase0=(inc * k) & 0xFFFFFFFFFFFFFFFF, sample0=k, **kw)
    assert np.array_equal(part.view(np.uint32), one[k:].view(np.uint32))


def test_in_place_one_tap(rx):
    rng = np.random.default_rng(3)
    n_rows, row_len = 6, 1473
    x = cnoise(rng, n_rows * row_len)
    kw = dict(taps=[[0.5 + 0.5j], [1.0], [-0.25j]], cfo=rng.uniform(-0.04, 0.04, n_rows).astype(np.float32), gain=3.0,
              noise_voltage=0.5, seed=17)
    want = run(rx, x, x.size, n_rows, row_len=row_len, **kw)
    buf = rx.alloc(x.nbytes).upload(x)
    rx.channel_dev(buf.ptr, buf.ptr, x.size, n_rows, row_len=row_len, **kw)
    got = buf.download(np.complex64, x.size)
    buf.free()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_argument_errors_launch_nothing(rx):
    lib = capi.lib()
    n_rows, row_len = 4, 100
    cap = n_rows * row_len + 16
    d_in = rx.alloc(cap * 8).upload(np.ones(cap, np.complex64))
    out = rx.alloc(cap * 8).upload(np.full(2 * cap, NAN_WORD, np.uint32))
    canary = out.download(np.uint8, cap * 8)
    taps = np.ones((2, 4), np.complex64)
    cfo = np.zeros(n_rows, np.float32)

    def call(i=-1, o=-1, cap=cap, row_off=None, row_len=row_len, n=n_rows, t=taps, L=4, sets=2, c=cfo, gain=1.0, nv=1.0):
        return lib.wifirx_channel(rx._h, d_in.ptr if i == -1 else i, out.ptr if o == -1 else o, cap, P(row_off), row_len, n,
                                  P(t), 0, L, sets, P(c), 0, gain, nv, 1, 0)

    bad_cfo = cfo.copy()
    bad_cfo[2] = np.nan
    cases = [
        (capi.EINVAL, dict(i=None)), (capi.EINVAL, dict(o=None)), (capi.EINVAL, dict(t=None)),
        (capi.EINVAL, dict(o=out.ptr + 4)), (capi.EINVAL, dict(L=0)), (capi.EINVAL, dict(L=65)), (capi.EINVAL, dict(sets=0)),
        (capi.EINVAL, dict(gain=math.inf)), (capi.EINVAL, dict(gain=math.nan)), (capi.EINVAL, dict(nv=-math.inf)),
        (capi.EINVAL, dict(nv=math.nan)), (capi.EINVAL, dict(c=bad_cfo)),
        (capi.EINVAL, dict(row_off=np.array([0, 100, 99, 200, 300], np.uint64))),
        (capi.EINVAL, dict(i=out.ptr)),                                    # in place with 4 taps
        (capi.EINVAL, dict(i=out.ptr + 8, L=1)),                           # overlapping, not the same buffer
        (capi.ERANGE, dict(cap=n_rows * row_len - 1)),
        (capi.ERANGE, dict(row_off=np.array([0, 100, 200, 300, cap + 1], np.uint64))),
    ]
    for code, kw in cases:
        assert call(**kw) == code, kw
    assert call(n=0) == capi.OK
    rx.sync()
    assert out.download(np.uint8, cap * 8).tobytes() == canary.tobytes(), "a refused call wrote samples"
    assert call(nv=0.0) == capi.OK
    rx.sync()
    got = out.download(np.complex64, cap)
    want = channel_ref.channel(np.ones((n_rows, row_len), np.complex64), taps=taps)
    assert np.array_equal(got[:n_rows * row_len], want.reshape(-1))
    d_in.free()
    out.free()


# ---- config 3 on the device: TX -> channel -> demod -> decode_mac ----

C3_SLOT, C3_LEAD, C3_ENC, C3_LEN, C3_FRAMES = 1472, 160, 7, 294, 30000


@pytest.mark.timeout(900)
@pytest.mark.parametrize("snr", [25, 30])
def test_config3_fer_against_the_oracle_table(orc, snr):
    import json
    table = {p["snr_db"]: p for p in json.load(open(os.path.join(GOLD, "config3_ber_table.json")))["points"]}
    n, seed = C3_FRAMES, 5000 + snr
    psdus = txgen.make_psdus(n, C3_LEN, seed=seed)                   # n distinct config-3 frames through the device chain
    taps = np.load(os.path.join(GOLD, "sv_taps.npy")).astype(np.complex64)
    cfo = np.random.default_rng(seed).uniform(-CFO_20PPM, CFO_20PPM, n).astype(np.float32)
    pick = np.sort(np.random.default_rng(seed + 1).choice(n, 256, replace=False))
    kw = dict(taps=taps, cfo=cfo, gain=math.sqrt(10 ** (snr / 10)), noise_voltage=1.0, seed=seed)
    (r, x), = loopback(psdus, C3_ENC, C3_LEAD, C3_SLOT, capi.EQ_LS, [kw], psdu_stride=304, pick=pick)
    crc = (r["frames"]["flags"] & capi.F_CRC_OK) != 0
    own = (r["psdu"][:, :C3_LEN] == psdus).all(axis=1)
    assert own[crc].all(), "a CRC-ok frame carries another PSDU"
    fer = 1.0 - float((crc & own).mean())
    ref = table[snr]["fer"]
    se = math.sqrt(fer * (1 - fer) / n + ref * (1 - ref) / table[snr]["frames"])
    assert abs(fer - ref) <= 4 * se, (snr, fer, ref, se)
    # the records and decisions of a subset against the oracle on the channel's own output
    assert_oracle_records(orc, r, x, C3_SLOT, pick, max_sym=txgen.n_sym_for(C3_LEN, C3_ENC))


# ---- IRS_tranceiver's loop-back through the blocks ----

def _chunks(rng, total, lo, hi):
    pos = 0
    while pos < total:
        n = int(min(rng.integers(lo, hi), total - pos))
        yield pos, n
        pos += n


def test_irs_tranceiver_chain_through_the_blocks():
    from wifirx import block, grshim
    rng = np.random.default_rng(2024)
    n_frames, enc = 200, 2
    sent = [txgen.mac_frame(rng.integers(0, 256, int(rng.integers(20, 400)), dtype=np.uint8).tobytes(), seq=k)
            for k in range(n_frames)]
    tx = block.wifi_phy_tx(encoding=enc, pad_front=100, pad_tail=1000)
    for p in sent:
        tx._handlers[grshim.intern("mac_in")](grshim.make_pdu({}, np.frombuffer(p, np.uint8)))
    parts = []
    while True:
        buf = np.empty(int(rng.integers(1, 50000)), np.complex64)
        n = tx.work([], [buf])
        if n == 0:
            break
        parts.append(buf[:n].copy())
    tx.close()
    x = np.concatenate(parts) * np.float32(math.sqrt(10 ** (25 / 10)))          # blocks.multiply_const_cc
    epsilon, freq = 10e-6, 5.89e9
    outs = []
    for lo, hi in ((1, 9000), (3000, 70000)):
        ch = block.channel_model(noise_voltage=1, frequency_offset=epsilon * freq / 10e6, epsilon=1.0, taps=[1.0],
                                 noise_seed=0)
        y = np.empty_like(x)
        for pos, n in _chunks(rng, x.size, lo, hi):
            assert ch.work([x[pos:pos + n]], [y[pos:pos + n]]) == n
        ch.close()
        outs.append(y)
    assert outs[0].tobytes() == outs[1].tobytes(), "channel_model output depends on the work() sizes"
    rx = block.wifi_phy_rx(bandwidth=20e6, frequency=5.89e9, publish_carrier=False)
    got = []
    grshim.msg_connect(rx, "mac_out", grshim.sink_block(got.append), "in")
    for pos, n in _chunks(rng, outs[0].size, 1, 30000):
        assert rx.work([outs[0][pos:pos + n]], []) == n
    rx.stop()
    rx.close()
    assert len(got) == n_frames, len(got)
    for k, (meta, vec) in enumerate(got):
        assert bytes(np.asarray(vec, np.uint8)) == sent[k][:-4], k
