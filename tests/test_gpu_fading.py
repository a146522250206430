"""wifirx_channel_fading, the channel with Doppler fading (wr_channel.hip, NUMERICS.md rule 19), on the device:
  * value for value tests/fading_ref.py without noise: rows that cross tile edges, 1, 8 and 16 taps, Doppler from 0 to the
    limit, Rayleigh and Rician, a stream time that puts the gains' grid off the row and tile starts, fixed rows and row_off
    rows, both output alignments; composed with the resampler of rule 18;
  * doppler NULL gives wifirx_channel_sro's bytes; with noise within rule 17's 1e-5; a row cut into two calls;
  * the host checks, before anything is queued; the stream block fed in uneven chunks;
  * 64-QAM 2/3 frames of 64 symbols through TX -> channel -> demod -> decode: at 1e-4 cycles per sample the LS equaliser loses
    the link and the STA equaliser keeps it."""
import math

import numpy as np
import pytest

import fading_ref
from channel_helpers import NAN_WORD, ONE, M64, P, assert_oracle_records, cnoise, loopback, run, rx, same, tap_sets  # noqa: F401 (rx: fixture)
from wifirx import block, capi, txgen

pytestmark = pytest.mark.gpu

FDS = np.array([0.0, 1e-5, 1e-4, 2.0 ** -10, 3e-4], np.float32)
TIMES = [0, (1 << 40) + 12345]


# ---- 1. noiseless, value for value ----

@pytest.mark.parametrize("L", [1, 8, 16])
@pytest.mark.parametrize("k_factor", [0.0, 10.0])
def test_noiseless_value_for_value_fixed_rows(rx, L, k_factor):
    """five rows of 4400 samples: two tile edges inside every row, every row with its own Doppler"""
    rng = np.random.default_rng(19 + L)
    x = cnoise(rng, 5 * 4400).reshape(5, 4400)
    cfo = np.array([0.037, -0.037, 0.011, -0.05, 0.002], np.float32)
    for time0 in TIMES:
        kw = dict(taps=tap_sets(rng, 2, L), cfo=cfo, phase0=0x0123456789ABCDEF, gain=0.5, doppler=FDS, k_factor=k_factor,
                  fade_seed=0xFEDCBA9876543210, time0=time0)
        want = fading_ref.channel(x, **kw)
        for shift in (0, 1):
            got = run(rx, x.reshape(-1), x.size, 5, shift, row_len=4400, **kw)
            assert same(got, want.reshape(-1)), (L, k_factor, time0, shift)


@pytest.mark.parametrize("L", [1, 8, 16])
@pytest.mark.parametrize("k_factor", [0.0, 10.0])
def test_noiseless_value_for_value_row_off(rx, L, k_factor):
    """odd row starts; an empty row, a 1-sample row and rows shorter than the taps; samples outside keep their NaNs"""
    rng = np.random.default_rng(300 + L)
    lens = [4400, 0, 1, 31, 7, 2049, 33, 0, 4097, 3]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(5)
    cap = int(off[-1]) + 7
    x = cnoise(rng, cap)
    fd = np.resize(FDS[[3, 1, 4, 2, 0]], len(lens))
    cfo = rng.uniform(-0.05, 0.05, len(lens)).astype(np.float32)
    inside = np.zeros(cap, bool)
    inside[int(off[0]):int(off[-1])] = True
    for time0 in TIMES:
        kw = dict(row_off=off, taps=tap_sets(rng, 2, L), cfo=cfo, gain=0.5, doppler=fd, k_factor=k_factor, fade_seed=7,
                  time0=time0)
        want = fading_ref.channel(x, **kw)
        for shift in (0, 1):
            got = run(rx, x, cap, len(lens), shift, **kw)
            assert same(got[inside], want[inside]), (L, k_factor, time0, shift)
            assert (got[~inside].view(np.uint32) == NAN_WORD).all(), (L, k_factor, time0, shift)


@pytest.mark.parametrize("k_factor", [0.0, 10.0])
def test_composed_with_the_resampler(rx, k_factor):
    """rule 18 in front of rule 19 in the one launch: +-20 ppm and the limit +-2^-8, a drift that starts off an integer"""
    rng = np.random.default_rng(1819)
    x = cnoise(rng, 5 * 4400).reshape(5, 4400)
    sro = np.array([20e-6, -20e-6, 2.0 ** -8, -2.0 ** -8, 0.0], np.float32)
    kw = dict(taps=tap_sets(rng, 2, 8), cfo=np.float32(0.011), phase0=99, sro=sro, drift0=int(0.37 * ONE) + 12345, gain=0.5,
              doppler=FDS, k_factor=k_factor, fade_seed=11, time0=TIMES[1])
    want = fading_ref.channel(x, **kw)
    for shift in (0, 1):
        got = run(rx, x.reshape(-1), x.size, 5, shift, row_len=4400, **kw)
        assert same(got, want.reshape(-1)), (k_factor, shift)


# ---- 2. the off switch, noise, a cut ----

@pytest.mark.parametrize("with_sro", [False, True])
def test_null_doppler_is_wifirx_channel_sro(rx, with_sro):
    rng = np.random.default_rng(5)
    n_rows, row_len, L = 5, 4400, 8
    x = cnoise(rng, n_rows * row_len)
    t = np.ascontiguousarray(tap_sets(rng, 2, L))
    c = rng.uniform(-0.05, 0.05, n_rows).astype(np.float32)
    s = np.array([20e-6, -20e-6, 2.0 ** -8, 0.0, -2.0 ** -8], np.float32) if with_sro else None
    lib = capi.lib()
    d_in = rx.alloc(x.nbytes).upload(x)
    outs = []
    for fading in (False, True):
        d_out = rx.alloc(x.nbytes).upload(np.full(2 * x.size, NAN_WORD, np.uint32))
        head = (rx._h, d_in.ptr, d_out.ptr, x.size, None, row_len, n_rows, P(t), 0, L, 2, P(c), 99, P(s), 12345, 1.7, 0.4, 3, 5)
        # k_factor, fade_seed and time0 are not looked at: not even a NaN k_factor is refused
        rc = lib.wifirx_channel_fading(*head, None, float("nan"), 77, 88) if fading else lib.wifirx_channel_sro(*head)
        assert rc == capi.OK
        outs.append(d_out.download(np.complex64, x.size))
        d_out.free()
    d_in.free()
    assert np.isfinite(outs[0]).all() and outs[1].tobytes() == outs[0].tobytes()


def test_noise_and_untouched_samples(rx):
    rng = np.random.default_rng(7)
    off = np.array([3, 1000, 1001, 3500, 3503, 8000], np.uint64)
    x = cnoise(rng, 8011)
    kw = dict(row_off=off, taps=tap_sets(rng, 2, 8), cfo=rng.uniform(-0.05, 0.05, 5).astype(np.float32), phase0=77, gain=2.0,
              noise_voltage=0.3, seed=99, sample0=12345, doppler=FDS, k_factor=10.0, fade_seed=99, time0=TIMES[1])
    want = fading_ref.channel(x, **kw)
    got = run(rx, x, 8011, 5, **kw)
    err = float(np.abs(got[3:8000] - want[3:8000]).max())
    print("distance from the restatement with noise: %.3e" % err)
    assert err <= 1e-5
    assert (got[:3].view(np.uint32) == NAN_WORD).all() and (got[8000:].view(np.uint32) == NAN_WORD).all()


@pytest.mark.parametrize("n_taps", [1, 8, 16])
def test_cut_invariance_on_the_device(rx, n_taps):
    rng = np.random.default_rng(40 + n_taps)
    n, k = 6000, 2345
    x = cnoise(rng, n)
    cfo = np.float32(0.021)
    inc = capi.phase_inc(cfo)
    kw = dict(taps=tap_sets(rng, 1, n_taps), cfo=cfo, gain=1.5, noise_voltage=0.3, seed=5, doppler=3e-4, k_factor=10.0, fade_seed=6)
    for time0 in TIMES:
        one = run(rx, x, n, 1, row_len=n, phase0=7, time0=time0, **kw)
        part = run(rx, x[k:], n - k, 1, row_len=n - k, phase0=(7 + inc * k) & M64, sample0=k, time0=time0 + k, **kw)
        assert part[n_taps - 1:].tobytes() == one[k + n_taps - 1:].tobytes(), time0


# ---- 3. the host checks ----

def test_host_checks_queue_nothing(rx):
    lib = capi.lib()
    n_rows, row_len = 4, 100
    cap = n_rows * row_len + 16
    x = cnoise(np.random.default_rng(3), cap)
    d_in = rx.alloc(cap * 8).upload(x)
    out = rx.alloc(cap * 8).upload(np.full(2 * cap, NAN_WORD, np.uint32))
    canary = out.download(np.uint8, cap * 8)
    taps = np.full((1, 17), 0.25, np.complex64)

    def call(fd, k_factor=0.0, n_taps=1, i=None, o=None, sro=None):
        t = np.ascontiguousarray(taps[:, :n_taps])
        return lib.wifirx_channel_fading(rx._h, d_in.ptr if i is None else i, out.ptr if o is None else o, cap, None, row_len,
                                         n_rows, P(t), 0, n_taps, 1, None, 0, P(sro), 0, 1.0, 0.0, 1, 0, P(fd), k_factor, 5, 9)

    def fd(v, at=2):
        d = np.full(n_rows, 1e-4, np.float32)
        d[at] = v
        return d

    over = np.nextafter(np.float32(2.0 ** -10), np.float32(1))
    cases = [
        dict(fd=fd(over)), dict(fd=fd(1e-3, at=3)), dict(fd=fd(-1e-9)), dict(fd=fd(-np.inf, at=0)), dict(fd=fd(np.inf)),
        dict(fd=fd(np.nan)),
        dict(fd=fd(1e-4), k_factor=-1.0), dict(fd=fd(1e-4), k_factor=float("nan")), dict(fd=fd(1e-4), k_factor=float("inf")),
        dict(fd=fd(1e-4), n_taps=17),
        dict(fd=fd(0.0), i=out.ptr),                                        # in place, one tap, no Doppler at all
        dict(fd=fd(1e-4), i=out.ptr),
        dict(fd=fd(1e-4), i=out.ptr + 8),                                   # overlapping
        dict(fd=fd(1e-4), i=out.ptr, sro=np.zeros(n_rows, np.float32)),
    ]
    for kw in cases:
        assert call(**kw) == capi.EINVAL, kw
    rx.sync()
    assert out.download(np.uint8, cap * 8).tobytes() == canary.tobytes(), "a refused call wrote samples"
    assert call(None, n_taps=17) == capi.OK                                 # without fading 17 taps are wifirx_channel's business
    # the largest values that pass: Doppler 2^-10 on every row, 16 taps, a huge K
    top = np.full(n_rows, 2.0 ** -10, np.float32)
    assert call(top, k_factor=3.0e38, n_taps=16) == capi.OK
    rx.sync()
    got = out.download(np.complex64, cap)[:n_rows * row_len].reshape(n_rows, row_len)
    want = fading_ref.channel(x[:n_rows * row_len].reshape(n_rows, row_len), taps=taps[:, :16], doppler=top, k_factor=3.0e38,
                              fade_seed=5, time0=9)
    assert same(got, want)
    d_in.free()
    out.free()


# ---- 4. the stream block ----

def test_block_in_uneven_chunks_equals_one_call(rx):
    rng = np.random.default_rng(12)
    n = 1000 + 4096 + 37 + 1000 + 37
    x = cnoise(rng, n)
    taps = tap_sets(rng, 1, 8)[0]
    kw = dict(doppler=2e-4, k_factor=10.0, fade_seed=21)
    want = rx.channel(x, taps=taps, cfo=np.float32(2.0 * math.pi * 1e-3), noise_voltage=0.2, seed=4, **kw)
    blk = block.channel_model(noise_voltage=0.2, frequency_offset=1e-3, taps=taps, noise_seed=4, **kw)
    try:
        got, at = np.zeros(n, np.complex64), 0
        for m in (1000, 4096, 37, 1000, 37):
            assert blk.work([x[at:at + m]], [got[at:at + m]]) == m
            at += m
    finally:
        blk.close()
    assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        block.channel_model(taps=np.ones(17), doppler=1e-4)
    # the defaults are today's block: no fader
    plain = block.channel_model(noise_voltage=0.2, frequency_offset=1e-3, taps=taps, noise_seed=4)
    try:
        y = np.zeros(1000, np.complex64)
        plain.work([x[:1000]], [y])
    finally:
        plain.close()
    assert y.tobytes() == rx.channel(x[:1000], taps=taps, cfo=np.float32(2.0 * math.pi * 1e-3), noise_voltage=0.2, seed=4).tobytes()


# ---- 5. end to end: which equaliser follows a channel that turns within the frame ----

def test_doppler_breaks_ls_and_not_sta_on_the_device(orc):
    e = fading_ref.E2E
    n, enc, plen, lead = e["n"], e["enc"], e["plen"], e["lead"]
    slot = lead + txgen.frame_samples(plen, enc) + 79
    psdus = txgen.make_psdus(n, plen, seed=e["psdu_seed"])
    res = {}
    for name, fd, eq in fading_ref.ARMS:
        kw = dict(gain=math.sqrt(10 ** (e["snr_db"] / 10)), noise_voltage=1.0, seed=e["seed"], doppler=fd, k_factor=e["k_factor"],
                  fade_seed=e["fade_seed"])
        res[name], = loopback(psdus, enc, lead, slot, eq, [kw], psdu_stride=1536)
    good = {name: int(((r["frames"]["flags"] & capi.F_CRC_OK) != 0).sum()) for name, (r, _) in res.items()}
    print("FCS-good of %d: %r" % (n, good))
    assert good["fd 1e-4, LS"] <= 15
    assert good["fd 1e-4, STA"] >= 40
    assert good["fd 0, LS"] >= 40
    # the records and decisions of the downloaded rows equal the oracle's
    for name, fd, eq in fading_ref.ARMS:
        assert_oracle_records(orc, *res[name], slot, msg=name, max_sym=txgen.n_sym_for(plen, enc), chan_est=eq)
