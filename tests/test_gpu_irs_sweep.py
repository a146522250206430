"""wifirx_irs_sweep, beam training of the reflecting surface over a codebook (wr_irs_sweep.hip, NUMERICS.md rule 26), on the device:
  * given scatter: power, winner and taps value for value tests/irs_sweep_ref.py, over odd N, the lane tail and several chunks,
    1 / 3 / 5 / 16 taps (16, 5, 3, 1 sets per tile), a ragged last tile, the column-tile tails of K, Rayleigh and Rician, with and
    without the direct path, the codebook on the host and on the device, scatter rows that wrap; the caps N = 4096 and K = 1024;
  * ties and NaN: the lower of two identical entries, an entry with a NaN never, all NaN gives 0;
  * Philox scatter: the elements are wifirx_irs_taps' for the same seed (the sweep exact on the device's own elements), and the
    winner's taps within the rule's bound of wifirx_irs_taps(psi = codebook[best]);
  * nothing written that was not asked for; the taps feed wifirx_channel on the device; block.channel_model(irs=IrsConfig(codebook=));
  * one end-to-end point: a link that a random configuration loses and the trained one keeps."""
import json
import math
import os

import numpy as np
import pytest

import channel_ref
import irs_sweep_ref as sr
from channel_helpers import cnoise, rx, same  # noqa: F401 (rx: fixture)
from wifirx import block, capi, irs, txgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def scene(rng, N, L, n_scatter):
    a, b, d = crandn(rng, N), crandn(rng, N), crandn(rng, 1)[0]
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    return a, b, d, pdp, crandn(rng, n_scatter, 2 * N + 1)


def book(rng, K, N):
    """K unit-modulus configurations: even entries of any phase, odd entries on the 2-bit table (exact zeros in either part)"""
    cb = np.exp(1j * rng.uniform(-np.pi, np.pi, (K, N))).astype(np.complex64)
    cb[1::2] = irs.quantize(cb[1::2], 2)
    return cb


def same_or_nan(got, want):
    """bit for bit where the restatement is a number, NaN where it is NaN (a NaN's payload is not part of the rule)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    g = got.view(np.float32) if np.iscomplexobj(got) else got
    w = want.view(np.float32) if np.iscomplexobj(want) else want
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and same(g[~nan], w[~nan])


def sweep(rx, n_sets, pdp, a, b, d, cb, cb_dev=False, **kw):
    d_cb = rx.alloc(cb.nbytes).upload(cb) if cb_dev else None
    try:
        return rx.irs_sweep(n_sets, pdp, a, b, d, codebook=d_cb if cb_dev else cb, **(dict(kw, n_codes=cb.shape[0]) if cb_dev else kw))
    finally:
        if d_cb is not None:
            d_cb.free()


# ---- 1. given scatter, value for value ----

#        N    L  n_sets K   k_factor direct cb_dev
CASES = [(1, 1, 1, 1, 0.0, 1.0, False),
         (2, 3, 7, 15, 10.0, 0.0, True),
         (3, 5, 7, 16, 0.0, 0.0, False),
         (63, 16, 7, 17, 10.0, 1.0, False),
         (64, 1, 7, 100, 10.0, 1.0, True),
         (64, 5, 7, 65, 10.0, 0.7, False),               # K = 65: the first entry of a wave's second group
         (65, 3, 7, 256, 0.0, 1.0, False),
         (130, 5, 1, 17, 10.0, 0.0, False),
         (257, 3, 7, 100, 10.0, 1.0, True),
         (4096, 2, 2, 17, 10.0, 1.0, False),             # the cap of N
         (65, 2, 2, 1024, 0.0, 1.0, True)]               # the cap of K


@pytest.mark.parametrize("N,L,n_sets,K,k_factor,dg,cb_dev", CASES)
def test_given_scatter_value_for_value(rx, N, L, n_sets, K, k_factor, dg, cb_dev):
    rng = np.random.default_rng(100000 * L + 1000 * K + N)
    n_scatter = max(1, n_sets * L - 2)                        # shorter than n_sets * L: the rows wrap
    a, b, d, pdp, sc = scene(rng, N, L, n_scatter)
    cb = book(rng, K, N)
    kw = dict(gain=1.3, k_factor=k_factor, direct_gain=dg, scatter=sc)
    want = sr.irs_sweep(n_sets, pdp, a, b, d, codebook=cb, **kw)
    got = sweep(rx, n_sets, pdp, a, b, d if dg else None, cb, cb_dev, **kw)
    assert same(got["power"], want["power"])
    assert np.array_equal(got["best"], want["best"]) and got["best"].dtype == np.uint16
    assert same(got["taps"], want["taps"])
    if N >= 63:                                               # (a few elements on the 2-bit table repeat their powers)
        assert np.unique(got["power"][0]).size == K           # the entries differ


# ---- 2. ties and NaN ----

def test_ties_and_nan_on_the_device(rx):
    N, L, n_sets = 65, 3, 7
    rng = np.random.default_rng(2)
    a, b, d, pdp, sc = scene(rng, N, L, n_sets * L)
    kw = dict(k_factor=3.0, scatter=sc)
    two = book(rng, 2, N)
    # two identical entries: the lower one wins (entries 0 = 3, 1 = 2, so every set's winner is 0 or 1)
    cb = np.stack([two[0], two[1], two[1], two[0]])
    got, want = sweep(rx, n_sets, pdp, a, b, d, cb, **kw), sr.irs_sweep(n_sets, pdp, a, b, d, codebook=cb, **kw)
    assert same(got["power"], want["power"]) and same(got["power"][:, 0], got["power"][:, 3]) and same(got["power"][:, 1], got["power"][:, 2])
    assert np.array_equal(got["best"], want["best"]) and (got["best"] < 2).all() and same(got["taps"], want["taps"])
    # an entry holding a NaN never wins, in the first place (nothing to beat yet) or the last
    for at in (0, 2):
        cb = np.stack([two[0], two[1], two[0]])
        cb[at, N // 2] = np.nan
        got, want = sweep(rx, n_sets, pdp, a, b, d, cb, **kw), sr.irs_sweep(n_sets, pdp, a, b, d, codebook=cb, **kw)
        assert np.isnan(got["power"][:, at]).all() and same_or_nan(got["power"], want["power"])
        assert np.array_equal(got["best"], want["best"]) and (got["best"] != at).all() and same(got["taps"], want["taps"])
    # all entries NaN: the winner is 0
    cb = np.stack([two[0], two[1], two[0]])
    cb[:, 5] = np.nan
    got, want = sweep(rx, n_sets, pdp, a, b, d, cb, **kw), sr.irs_sweep(n_sets, pdp, a, b, d, codebook=cb, **kw)
    assert np.isnan(got["power"]).all() and (got["best"] == 0).all() and (want["best"] == 0).all()
    assert np.isnan(got["taps"]).all()


# ---- 3. Philox scatter ----

@pytest.mark.parametrize("N,L,n_sets,K", [(65, 3, 7, 17), (300, 2, 5, 100)])
def test_philox_scatter(rx, N, L, n_sets, K):
    rng = np.random.default_rng(N)
    a, b, d, pdp, _ = scene(rng, N, L, 1)
    cb = book(rng, K, N)
    seed = 0xFEDCBA9876543210
    scale = np.sqrt(pdp.astype(np.float64)).astype(np.float32)
    for k_factor in (0.0, 10.0):
        # the same seed: wifirx_irs_taps hands out the elements the sweep uses.  The direct path is blocked, as in
        # test_gpu_irs.py (it would be one more draw through the device's own Box-Muller)
        kw = dict(k_factor=k_factor, direct_gain=0.0, seed=seed)
        el = rx.irs_taps(n_sets, pdp, a, b, None, psi=np.ones(N, np.complex64), want_elems=True, **kw)["elems"]
        got = sweep(rx, n_sets, pdp, a, b, None, cb, **kw)
        want = sr.irs_sweep(n_sets, pdp, a, b, None, codebook=cb, elems=el, **kw)
        assert same(got["power"], want["power"]) and np.array_equal(got["best"], want["best"]) and same(got["taps"], want["taps"])
        # rule 25 with the winner's configuration: the same value rounded in another order
        other = rx.irs_taps(n_sets, pdp, a, b, None, psi=cb[got["best"]], **kw)
        lim = sr.bound(np.zeros((n_sets, L)), el[:, :, 0, :], el[:, :, 1, :], scale)
        err = np.abs(got["taps"].astype(np.complex128) - other.astype(np.complex128))
        print("N = %d, K = %g: winner's taps against wifirx_irs_taps, largest error / bound = %.4f" % (N, k_factor, float((err / lim).max())))
        assert (err <= lim).all()


# ---- 4. outputs that were not asked for; into the channel ----

def test_nothing_beyond_what_was_asked_for(rx):
    N, L, n_sets, K, guard = 65, 3, 7, 17, 64
    rng = np.random.default_rng(4)
    a, b, d, pdp, _ = scene(rng, N, L, 1)
    cb = book(rng, K, N)
    sizes = {"taps": n_sets * L * 8, "best": n_sets * 2, "power": n_sets * K * 4}
    full = None
    for leave in (None, "taps", "best", "power"):
        bufs = {k: rx.alloc(v + guard).upload(np.full(v + guard, 0xA5, np.uint8)) for k, v in sizes.items()}
        ptr = {k: (None if k == leave else bufs[k]) for k in sizes}
        rx.irs_sweep_dev(ptr["taps"], n_sets, pdp, a, b, d, codebook=cb, k_factor=3.0, seed=9, best_ptr=ptr["best"], power_ptr=ptr["power"])
        got = {k: bufs[k].download(np.uint8, v + guard) for k, v in sizes.items()}
        for buf in bufs.values():
            buf.free()
        if leave is None:
            full = got
        for k, v in sizes.items():
            assert (got[k][v:] == 0xA5).all(), (leave, k, "the guard region")
            if k == leave:
                assert (got[k][:v] == 0xA5).all(), (leave, "written without being asked for")
            else:
                assert got[k][:v].tobytes() == full[k][:v].tobytes(), (leave, k, "depends on which outputs are asked for")
    assert np.isfinite(full["taps"][:sizes["taps"]].view(np.complex64)).all()
    assert (full["best"][:sizes["best"]].view(np.uint16) < K).all()


def test_winners_feed_the_channel_on_the_device(rx):
    n_rows, row_len, S, L = 5, 200, 8, 8
    rng = np.random.default_rng(6)
    x = cnoise(rng, n_rows * row_len).reshape(n_rows, row_len)
    b2r, r2u, b2u = irs.los(S, [0.015, 0.015, 0], [0.12, 0.12, 4.5], [0.42, -0.08, 1.0])
    cb = irs.dft_codebook(S, b2r, over=1, bits=2)
    pdp = np.exp(-np.arange(L) / 2.0)
    d_taps, d_in, d_out = rx.alloc(n_rows * L * 8), rx.alloc(x.nbytes).upload(x), rx.alloc(x.nbytes)
    try:
        rx.irs_sweep_dev(d_taps, n_rows, pdp / pdp.sum(), b2r, r2u, b2u, codebook=cb, gain=1.0 / S, k_factor=10.0, seed=3)
        rx.channel_dev(d_in.ptr, d_out.ptr, x.size, n_rows, row_len=row_len, taps=d_taps.ptr, n_taps=L, n_tap_sets=n_rows,
                       cfo=np.float32(0.01))
        taps = d_taps.download(np.complex64, n_rows * L).reshape(n_rows, L)
        y = d_out.download(np.complex64, x.size).reshape(n_rows, row_len)
    finally:
        for buf in (d_taps, d_in, d_out):
            buf.free()
    assert np.isfinite(taps).all() and len(np.unique(taps)) == taps.size
    assert same(y, channel_ref.channel(x, taps=taps, cfo=np.float32(0.01)))


def test_block_with_a_trained_surface(rx):
    cfg = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0), k_factor=5.0,
               pdp=(0.6, 0.3, 0.1), seed=11, refresh=1500)
    cb = irs.dft_codebook(4, over=2, bits=2)
    n = 1000 + 4096 + 37
    x = cnoise(np.random.default_rng(12), n)
    c = irs.IrsConfig(codebook=cb, **cfg)
    direct = rx.irs_sweep(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, codebook=cb, k_factor=5.0, seed=11)
    sets = direct["taps"]
    coef = [(sets[np.arange(n) // 1500, l].real.copy(), sets[np.arange(n) // 1500, l].imag.copy()) for l in range(3)]
    want = channel_ref.mix(*channel_ref.fir(x, coef), inc=channel_ref.phase_inc(np.float32(0.0)), noise_voltage=0.0)
    blk = block.channel_model(noise_voltage=0.0, irs=c)
    try:
        assert blk.irs_best.size == 0
        got, at = np.zeros(n, np.complex64), 0
        for m in (1000, 4096, 37):
            assert blk.work([x[at:at + m]], [got[at:at + m]]) == m
            at += m
        best = blk.irs_best
        with pytest.raises(ValueError):
            blk.set_psi(np.ones(16))
    finally:
        blk.close()
    assert same(got, want)
    assert best.dtype == np.uint16 and best.size >= n // 1500 + 1 and np.array_equal(best[:16], direct["best"][:best.size][:16])


# ---- 5. one end-to-end point (tests/irs_sweep_point.py chose it on the host) ----

def test_training_closes_a_link_a_random_configuration_cannot(rx, orc):
    import irs_sweep_point as pt
    from channel_helpers import assert_oracle_records, loopback
    with open(os.path.join(ROOT, "profiles", "irs_sweep_operating_point.json")) as f:
        rec = json.load(f)
    point = [p for p in rec["points"] if p["snr_db"] == rec["chosen_snr_db"]][0]
    assert rec["chosen_snr_db"] == pt.SNR_DB and point["accepted"]
    assert point["random"] <= pt.RANDOM_AT_MOST and point["sweep"] >= pt.SWEEP_AT_LEAST
    n = pt.N_FRAMES
    n_sym, slot = pt.geometry()
    b2r, r2u = pt.scene()
    psdus = txgen.make_psdus(n, pt.PLEN, seed=pt.PSDU_SEED)
    sets = {arm: rx.alloc(n * 8) for arm in pt.ARMS}
    d_best = rx.alloc(n * 2)
    try:
        rx.irs_taps_dev(sets["random"], n, [1.0], b2r, r2u, None, **pt.surface("random"))
        rx.irs_sweep_dev(sets["sweep"], n, [1.0], b2r, r2u, None, best_ptr=d_best, **pt.surface("sweep"))
        best = d_best.download(np.uint16, n)
        rx.sync()                                             # the loop-back runs on a handle of its own
        noise = dict(gain=math.sqrt(10 ** (pt.SNR_DB / 10)), noise_voltage=1.0, seed=pt.NOISE_SEED)
        chans = [dict(taps=sets[arm].ptr, n_taps=1, n_tap_sets=n, **noise) for arm in pt.ARMS]
        res = loopback(psdus, pt.ENC, pt.LEAD, slot, capi.EQ_LS, chans, psdu_stride=112)
    finally:
        for buf in sets.values():
            buf.free()
        d_best.free()
    good = {arm: int(((r["frames"]["flags"] & capi.F_CRC_OK) != 0).sum()) for arm, (r, _) in zip(pt.ARMS, res)}
    print("FCS-good of %d at %g dB per path: %r (host chain: random %d, sweep %d); %d distinct winners"
          % (n, pt.SNR_DB, good, point["random"], point["sweep"], np.unique(best).size))
    # the device's elements differ from the host's in the last bits of the Box-Muller (rule 17's 1e-5), so a frame on the edge
    # may fall the other way: the counts are held to the acceptance limits, not to the host's exact numbers
    assert good["random"] <= pt.RANDOM_AT_MOST
    assert good["sweep"] >= pt.SWEEP_AT_LEAST
    for arm, (r, x) in zip(pt.ARMS, res):
        assert_oracle_records(orc, r, x, slot, msg=arm, max_sym=n_sym)
