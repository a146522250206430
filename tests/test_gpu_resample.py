"""wifirx_channel_sro, the channel with a sample-rate offset (wr_channel.hip, NUMERICS.md rule 18), on the device:
  * value for value tests/resample_ref.py without noise: rows that cross tile edges, drifts that cross integer boundaries,
    1 and 8 taps, fixed rows and row_off rows (empty, 1 sample, shorter than the resampler), both output alignments;
  * with noise within rule 17's 1e-5, and nothing written outside the rows;
  * no resampling (sro NULL, or all-zero sro and drift0 = 0) gives wifirx_channel's bytes;
  * the host checks, before anything is queued; a row cut into two calls;
  * 64-QAM 3/4 frames of 57 symbols at +-20 ppm through TX -> channel -> demod -> decode with the LS equaliser: they
    decode with the sample clock locked to the carrier and not without."""
import math

import numpy as np
import pytest

import resample_ref
from channel_helpers import NAN_WORD, ONE, M64, P, assert_oracle_records, cnoise, loopback, run, rx, tap_sets  # noqa: F401 (rx: fixture)
from wifirx import capi, txgen

pytestmark = pytest.mark.gpu

SROS = np.array([0.0, 20e-6, -20e-6, 2.0 ** -8, -2.0 ** -8], np.float32)
DRIFTS = [0, int(0.37 * ONE) + 12345, -(3 * ONE + ONE // 4)]


@pytest.fixture(scope="module")
def fixed_rows():
    """five rows of 4400 samples (two tile edges inside) and their restatement for every (drift0, n_taps)"""
    rng = np.random.default_rng(18)
    x = cnoise(rng, 5 * 4400).reshape(5, 4400)
    cfo = np.array([0.037, -0.037, 0.011, -0.05, 0.002], np.float32)
    cases = {}
    for L in (1, 8):
        taps = tap_sets(rng, 2, L)
        for d0 in DRIFTS:
            kw = dict(taps=taps, cfo=cfo, phase0=0x0123456789ABCDEF, sro=SROS, drift0=d0, gain=0.5)
            cases[L, d0] = (kw, resample_ref.channel(x, **kw))
    return x, cases


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("d0", DRIFTS)
def test_noiseless_value_for_value_fixed_rows(rx, fixed_rows, L, d0):
    x, cases = fixed_rows
    kw, want = cases[L, d0]
    # the drift of the steepest rows crosses 17 integer boundaries
    assert abs((d0 + resample_ref.drift_inc(SROS[3]) * 4399 >> 40) - (d0 >> 40)) == 17
    for shift in (0, 1):
        got = run(rx, x.reshape(-1), x.size, 5, shift, row_len=4400, **kw)
        assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)), (L, d0, shift)


@pytest.mark.parametrize("L", [1, 8])
def test_noiseless_value_for_value_row_off(rx, L):
    """odd row starts; an empty row, a 1-sample row and rows shorter than the resampler; samples outside keep their NaNs"""
    rng = np.random.default_rng(200 + L)
    lens = [4400, 0, 1, 31, 7, 2049, 33, 0, 4097, 3]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64) + np.uint64(5)
    cap = int(off[-1]) + 7
    x = cnoise(rng, cap)
    sro = np.resize(SROS[[3, 1, 4, 2, 0]], len(lens))
    cfo = rng.uniform(-0.05, 0.05, len(lens)).astype(np.float32)
    inside = np.zeros(cap, bool)
    inside[int(off[0]):int(off[-1])] = True
    for d0 in DRIFTS:
        kw = dict(row_off=off, taps=tap_sets(rng, 2, L), cfo=cfo, sro=sro, drift0=d0, gain=0.5)
        want = resample_ref.channel(x, **kw)
        for shift in (0, 1):
            got = run(rx, x, cap, len(lens), shift, **kw)
            assert np.array_equal(got[inside].view(np.uint32), want[inside].view(np.uint32)), (L, d0, shift)
            assert (got[~inside].view(np.uint32) == NAN_WORD).all(), (L, d0, shift)


def test_noise_and_untouched_samples(rx):
    rng = np.random.default_rng(7)
    off = np.array([3, 1000, 1001, 3500, 3503, 8000], np.uint64)
    x = cnoise(rng, 8011)
    kw = dict(row_off=off, taps=tap_sets(rng, 2, 8), cfo=rng.uniform(-0.05, 0.05, 5).astype(np.float32), phase0=77,
              sro=SROS, drift0=DRIFTS[1], gain=2.0, noise_voltage=0.3, seed=99, sample0=12345)
    want = resample_ref.channel(x, **kw)
    got = run(rx, x, 8011, 5, **kw)
    err = float(np.abs(got[3:8000] - want[3:8000]).max())
    print("distance from the restatement with noise: %.3e" % err)
    assert err <= 1e-5
    assert (got[:3].view(np.uint32) == NAN_WORD).all() and (got[8000:].view(np.uint32) == NAN_WORD).all()


@pytest.mark.parametrize("L", [1, 8])
def test_no_resampling_is_wifirx_channel(rx, L):
    rng = np.random.default_rng(L)
    n_rows, row_len = 5, 4400
    x = cnoise(rng, n_rows * row_len)
    kw = dict(row_len=row_len, taps=tap_sets(rng, 2, L), cfo=rng.uniform(-0.05, 0.05, n_rows).astype(np.float32),
              phase0=99, gain=1.7, noise_voltage=0.4, seed=3, sample0=5)
    base = run(rx, x, x.size, n_rows, **kw)
    assert np.isfinite(base).all()
    zero = run(rx, x, x.size, n_rows, sro=np.zeros(n_rows, np.float32), drift0=0, **kw)
    assert zero.tobytes() == base.tobytes()
    # sro = NULL through wifirx_channel_sro itself (drift0 is then not looked at)
    d_in = rx.alloc(x.nbytes).upload(x)
    d_out = rx.alloc(x.nbytes).upload(np.full(2 * x.size, NAN_WORD, np.uint32))
    t, c = np.ascontiguousarray(kw["taps"]), kw["cfo"]
    rc = capi.lib().wifirx_channel_sro(rx._h, d_in.ptr, d_out.ptr, x.size, None, row_len, n_rows, P(t), 0, L, 2, P(c), 99, None,
                                       123456789, 1.7, 0.4, 3, 5)
    assert rc == capi.OK
    null = d_out.download(np.complex64, x.size)
    d_in.free()
    d_out.free()
    assert null.tobytes() == base.tobytes()


def test_host_checks_queue_nothing(rx):
    lib = capi.lib()
    n_rows, row_len = 4, 100
    cap = n_rows * row_len + 16
    d_in = rx.alloc(cap * 8).upload(np.ones(cap, np.complex64))
    out = rx.alloc(cap * 8).upload(np.full(2 * cap, NAN_WORD, np.uint32))
    canary = out.download(np.uint8, cap * 8)
    taps = np.ones((1, 1), np.complex64)

    def call(sro, i=None, o=None, drift0=0, row_off=None):
        return lib.wifirx_channel_sro(rx._h, d_in.ptr if i is None else i, out.ptr if o is None else o, cap, P(row_off), row_len,
                                      n_rows, P(taps), 0, 1, 1, None, 0, P(sro), drift0, 1.0, 0.0, 1, 0)

    def sro(v, at=2):
        s = np.zeros(n_rows, np.float32)
        s[at] = v
        return s

    over = np.nextafter(np.float32(2.0 ** -8), np.float32(1))
    cases = [
        (capi.EINVAL, dict(sro=sro(over))), (capi.EINVAL, dict(sro=sro(-over))), (capi.EINVAL, dict(sro=sro(0.5, at=3))),
        (capi.EINVAL, dict(sro=sro(np.nan))), (capi.EINVAL, dict(sro=sro(np.inf))), (capi.EINVAL, dict(sro=sro(-np.inf, at=0))),
        (capi.EINVAL, dict(sro=sro(0.0), i=out.ptr)),                       # in place, one tap, no drift at all
        (capi.EINVAL, dict(sro=sro(20e-6), i=out.ptr)),
        (capi.EINVAL, dict(sro=sro(20e-6), i=out.ptr + 8)),                 # overlapping
        (capi.ERANGE, dict(sro=sro(2.0 ** -8), drift0=(1 << 62) - (100 << 32) + 1)),
        (capi.ERANGE, dict(sro=sro(-2.0 ** -8), drift0=-(1 << 62))),
        (capi.ERANGE, dict(sro=sro(0.0), drift0=1 << 62)),
        (capi.ERANGE, dict(sro=sro(0.0), drift0=-(1 << 63))),
        (capi.ERANGE, dict(sro=sro(2.0 ** -8), drift0=(1 << 62) - (300 << 32),
                           row_off=np.array([0, 0, 5, 405, 410], np.uint64))),          # the longest row decides
    ]
    for code, kw in cases:
        assert call(**kw) == code, kw
    rx.sync()
    assert out.download(np.uint8, cap * 8).tobytes() == canary.tobytes(), "a refused call wrote samples"
    # the largest values that pass
    assert call(sro(2.0 ** -8), drift0=(1 << 62) - (100 << 32) - 1) == capi.OK
    assert call(sro(-2.0 ** -8), drift0=0) == capi.OK
    rx.sync()
    got = out.download(np.complex64, cap)[:n_rows * row_len].reshape(n_rows, row_len)
    want = resample_ref.channel(np.ones((n_rows, row_len), np.complex64), sro=sro(-2.0 ** -8), drift0=0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    d_in.free()
    out.free()


@pytest.mark.parametrize("n_taps", [1, 8])
def test_cut_invariance_on_the_device(rx, n_taps):
    rng = np.random.default_rng(40 + n_taps)
    n, k = 6000, 2345
    x = cnoise(rng, n)
    taps = tap_sets(rng, 1, n_taps)
    cfo = np.float32(0.021)
    inc = capi.phase_inc(cfo)
    d0 = int(0.4 * ONE)
    halo = 31 + n_taps
    for s in SROS[1:3]:
        dinc = capi.drift_inc(s)
        kw = dict(taps=taps, cfo=cfo, sro=s, gain=1.5, noise_voltage=0.3, seed=5)
        one = run(rx, x, n, 1, row_len=n, phase0=7, drift0=d0, **kw)
        part = run(rx, x[k:], n - k, 1, row_len=n - k, phase0=(7 + inc * k) & M64, drift0=d0 + dinc * k,
                   sample0=k, **kw)
        assert part[halo:].tobytes() == one[k + halo:].tobytes(), float(s)


# ---- end to end: the receiver's sampling-offset compensation meets a channel that drifts ----

def test_long_frames_decode_with_the_locked_clock_only(orc):
    n, enc, plen, lead = 48, 7, 1528, 160
    slot = lead + txgen.frame_samples(plen, enc) + 79
    psdus = txgen.make_psdus(n, plen, seed=18)
    cfo = np.where(np.arange(n) % 2 == 0, 0.037, -0.037).astype(np.float32)
    arms = {"locked": capi.locked_sro(cfo), "unlocked": None}
    res = loopback(psdus, enc, lead, slot, capi.EQ_LS, psdu_stride=1536, channels=[
        dict(cfo=cfo, sro=sro, gain=math.sqrt(10 ** 3.2), noise_voltage=1.0, seed=32) for sro in arms.values()])
    good = {name: int(((r["frames"]["flags"] & capi.F_CRC_OK) != 0).sum()) for name, (r, _) in zip(arms, res)}
    print("FCS-good of %d: %r" % (n, good))
    assert good["locked"] >= 45
    assert good["unlocked"] <= 3
    # the records of the downloaded rows equal the oracle's
    for name, (r, x) in zip(arms, res):
        assert_oracle_records(orc, r, x, slot, msg=name, max_sym=txgen.n_sym_for(plen, enc), chan_est=capi.EQ_LS)
