"""wifirx_irs_taps, the reflecting surface's cascade channel (wr_irs.hip, NUMERICS.md rule 25), on the device:
  * given scatter: value for value tests/irs_ref.py, over the lane tail, one pass, the second pass, a ragged one and the cap of
    4096 elements, 1 / 3 / 16 taps, psi sets and scatter rows that wrap, Rayleigh and Rician, with and without the direct
    path, psi on the host and on the device; the reference's own channel (tests/golden/irs_reference.npz) within the rule's bound;
  * the aligned mode: codes and taps bit for bit, B = 1, 2, 3, the codes of a set whatever its tap count;
  * Philox scatter: the elements within rule 17's 1e-5 of the restatement, the rest of the chain exact on the device's own
    elements, the same bytes from the same seed, other draws from another seed, set or tap, no correlation with the noise;
  * nothing written that was not asked for; the sets feed wifirx_channel on the device; block.channel_model(irs=...);
  * one end-to-end point: a link that is lost without the surface, kept with the aligned one."""
import json
import math
import os

import numpy as np
import pytest

import channel_ref
import irs_ref
from channel_helpers import NAN_WORD, cnoise, rx, same  # noqa: F401 (rx: fixture)
from wifirx import block, capi, irs, txgen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "irs_reference.npz")
SIZES = [1, 63, 64, 65, 130, 4096]


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def scene(rng, N, L, n_scatter):
    a, b, d = crandn(rng, N), crandn(rng, N), crandn(rng, 1)[0]
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    return a, b, d, pdp, crandn(rng, n_scatter, 2 * N + 1)


# ---- 1. given scatter, value for value ----

@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("L", [1, 3, 16])
def test_given_scatter_value_for_value(rx, N, L):
    rng = np.random.default_rng(1000 * L + N)
    for n_sets, n_psi, k_factor, dg, psi_dev in [(1, 1, 0.0, 1.0, False), (5, 2, 10.0, 0.0, True), (5, 1, 10.0, 1.0, False),
                                                 (5, 2, 0.0, 0.0, False)]:
        n_scatter = max(1, n_sets * L - 2)                    # shorter than n_sets * L: the rows wrap
        a, b, d, pdp, sc = scene(rng, N, L, n_scatter)
        psi = np.stack([irs.random_psi(N, 3, 7), (crandn(rng, N) * np.float32(0.8)).astype(np.complex64)])[:n_psi]
        kw = dict(gain=1.3, k_factor=k_factor, direct_gain=dg)
        want = irs_ref.irs_taps(n_sets, pdp, a, b, d, psi=psi, scatter=sc, **kw)
        d_psi = rx.alloc(psi.nbytes).upload(psi) if psi_dev else None
        try:
            got = rx.irs_taps(n_sets, pdp, a, b, d, psi=d_psi if psi_dev else psi, n_psi_sets=n_psi, scatter=sc, want_elems=True, **kw)
        finally:
            if d_psi is not None:
                d_psi.free()
        assert same(got["elems"], want["elems"]), (n_sets, n_psi, k_factor, dg)
        assert same(got["taps"], want["taps"]), (n_sets, n_psi, k_factor, dg)


def test_reference_fixture_on_the_device(rx):
    """the reference's draws, K = 10 and psi through the kernel: within rule 25's bound of Channel.getChnl's H"""
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for S in (2, 4, 16):
        N = S * S
        for u in range(2):
            tag = "S%d_u%d" % (S, u)
            nlos, mixes, H = g["nlos_" + tag], g["mix_" + tag], g["H_" + tag]
            lim = irs_ref.bound(mixes[:, 2 * N], mixes[:, :N], mixes[:, N:2 * N])
            for j in range(2):
                got = rx.irs_taps(nlos.shape[0], [1.0], g["los_%s_b2r" % tag], g["los_%s_r2u" % tag], g["los_%s_b2u" % tag],
                                  k_factor=float(g["k_factor"]), psi=g["psi_S%d" % S][j], scatter=nlos)
                err = np.abs(got[:, 0].astype(np.complex128) - H[:, j])
                print("S = %d, user %d, psi %d: largest error / bound = %.3f" % (S, u, j, float((err / lim).max())))
                assert (err <= lim).all(), (S, u, j)


# ---- 2. the aligned mode ----

@pytest.mark.parametrize("bits", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 300, 4096])
def test_aligned_mode_value_for_value(rx, bits, N):
    rng = np.random.default_rng(50 * bits + N)
    L, n_sets = 3, 4
    a, b, d, pdp, sc = scene(rng, N, L, n_sets * L)
    for dg, k_factor in [(1.0, 10.0), (0.0, 0.0), (0.7, 0.0)]:
        kw = dict(k_factor=k_factor, direct_gain=dg, align_bits=bits, scatter=sc)
        want = irs_ref.irs_taps(n_sets, pdp, a, b, d, **kw)
        got = rx.irs_taps(n_sets, pdp, a, b, d if dg else None, want_codes=True, **kw)
        assert np.array_equal(got["codes"], want["codes"]), (dg, k_factor)
        assert same(got["taps"], want["taps"]), (dg, k_factor)
        assert got["codes"].max() < (1 << bits)
        if N > 1:
            assert len(np.unique(got["codes"])) == (1 << bits)
    # the codes of a set do not depend on how many taps it is run with (scatter rows chosen so that tap 0 reads the same row)
    one = rx.irs_taps(n_sets, pdp[:1], a, b, d, k_factor=10.0, align_bits=bits, scatter=sc[::L], want_codes=True)
    all_taps = rx.irs_taps(n_sets, pdp, a, b, d, k_factor=10.0, align_bits=bits, scatter=sc, want_codes=True)
    assert np.array_equal(one["codes"], all_taps["codes"]) and same(one["taps"][:, 0], all_taps["taps"][:, 0])


# ---- 3. Philox scatter ----

@pytest.mark.parametrize("N,L,n_sets", [(65, 3, 5), (4096, 2, 2)])
def test_philox_scatter(rx, N, L, n_sets):
    rng = np.random.default_rng(N)
    a, b, d, pdp, _ = scene(rng, N, L, 1)
    psi = irs.random_psi(N, 2, 3)
    seed = 0xFEDCBA9876543210
    for k_factor in (0.0, 10.0):
        kw = dict(k_factor=k_factor, psi=psi, seed=seed)
        want = irs_ref.irs_taps(n_sets, pdp, a, b, d, **kw)
        got = rx.irs_taps(n_sets, pdp, a, b, d, want_elems=True, **kw)
        err = float(np.abs(got["elems"] - want["elems"]).max())
        print("N = %d, K = %g: elements within %.3e of the restatement" % (N, k_factor, err))
        assert err <= 1e-5
        # the rest of the chain on the device's own elements, the direct path blocked (it would be one more draw): exact
        g0 = rx.irs_taps(n_sets, pdp, a, b, None, direct_gain=0.0, want_elems=True, **kw)
        assert same(g0["elems"], got["elems"])
        assert same(g0["taps"], irs_ref.irs_taps(n_sets, pdp, a, b, None, direct_gain=0.0, elems=g0["elems"], **kw)["taps"])
        for bits in (1, 2, 3):
            ka = dict(k_factor=k_factor, align_bits=bits, seed=seed, direct_gain=0.0)
            ga = rx.irs_taps(n_sets, pdp, a, b, None, want_elems=True, want_codes=True, **ka)
            wa = irs_ref.irs_taps(n_sets, pdp, a, b, None, elems=ga["elems"], **ka)
            assert same(ga["elems"], got["elems"]) and np.array_equal(ga["codes"], wa["codes"]) and same(ga["taps"], wa["taps"])
        # with the direct path: one more Box-Muller sample of at most unit scale (1e-5) times a tap scale of at most 1, and
        # the one rounding of h_d + sum that it may move (an ulp of the tap, 2^-23 of its magnitude)
        rest = irs_ref.irs_taps(n_sets, pdp, a, b, d, elems=got["elems"], **kw)
        assert float(np.abs(got["taps"] - rest["taps"]).max()) <= 1e-5 + 2.0 ** -23 * float(np.abs(rest["taps"]).max())


def test_philox_seeds_sets_and_taps(rx):
    N, L, n_sets = 130, 3, 4
    one = np.ones(N, np.complex64)
    kw = dict(psi=one, want_elems=True)
    r1 = rx.irs_taps(n_sets, np.ones(L), one, one, 1.0, seed=5, **kw)
    r2 = rx.irs_taps(n_sets, np.ones(L), one, one, 1.0, seed=5, **kw)
    assert r1["taps"].tobytes() == r2["taps"].tobytes() and r1["elems"].tobytes() == r2["elems"].tobytes()
    r3 = rx.irs_taps(n_sets, np.ones(L), one, one, 1.0, seed=5 + (1 << 32), **kw)
    assert not np.array_equal(r1["elems"], r3["elems"])
    e = np.concatenate([r1["elems"].reshape(-1), r3["elems"].reshape(-1)])
    assert np.unique(e).size == e.size                        # every (seed, r, l, leg, n) its own draw
    assert np.isfinite(e).all() and abs(float((np.abs(e) ** 2).mean()) - 1.0) < 0.05
    # the same value as seed of the channel's noise: counter word 3 keeps the two sequences apart
    n = 2 * L * N                                             # the elements of set 0 as a sequence
    z = np.zeros(n, np.complex64)
    w = rx.channel(z, noise_voltage=1.0, seed=5)
    v = r1["elems"][0].reshape(-1)
    rho = np.vdot(v - v.mean(), w - w.mean()) / (n * v.std() * w.std())
    print("sample correlation with the channel's noise: %.4f (5 / sqrt(n) = %.4f)" % (abs(rho), 5 / math.sqrt(n)))
    assert abs(rho) <= 5 / math.sqrt(n)


# ---- 4. outputs that were not asked for ----

def test_nothing_beyond_what_was_asked_for(rx):
    N, L, n_sets, guard = 65, 3, 5, 64
    rng = np.random.default_rng(4)
    a, b, d, pdp, _ = scene(rng, N, L, 1)
    sizes = {"taps": n_sets * L * 8, "elems": n_sets * L * 2 * N * 8, "codes": n_sets * N}
    for bits, want in [(0, ()), (2, ()), (2, ("codes",)), (0, ("elems",)), (2, ("elems", "codes"))]:
        bufs = {k: rx.alloc(v + guard).upload(np.full(v + guard, 0xA5, np.uint8)) for k, v in sizes.items()}
        rx.irs_taps_dev(bufs["taps"], n_sets, pdp, a, b, d, k_factor=3.0, psi=None if bits else irs.random_psi(N, 2, 1), align_bits=bits,
                        seed=9, elems_ptr=bufs["elems"] if "elems" in want else None, codes_ptr=bufs["codes"] if "codes" in want else None)
        for k, v in sizes.items():
            got = bufs[k].download(np.uint8, v + guard)
            assert (got[v:] == 0xA5).all(), (bits, want, k, "the guard region")
            if k == "taps":
                assert np.isfinite(got[:v].view(np.complex64)).all()
            elif k not in want:
                assert (got[:v] == 0xA5).all(), (bits, want, k, "written without being asked for")
            else:
                assert (got[:v] != 0xA5).any()
            bufs[k].free()


# ---- 6. one end-to-end point (tests/irs_point.py chose it on the host) ----

def test_surface_closes_a_link_the_direct_path_cannot(rx, orc):
    import irs_point as pt
    from channel_helpers import assert_oracle_records, loopback
    n = pt.N_FRAMES
    n_sym, slot = pt.geometry()
    psdus = txgen.make_psdus(n, pt.PLEN, seed=pt.PSDU_SEED)
    one = np.ones(pt.N_ELEMS, np.complex64)
    sets = {arm: rx.alloc(n * 8) for arm in pt.ARMS[1:]}
    try:
        for arm, buf in sets.items():
            rx.irs_taps_dev(buf, n, [1.0], one, one, None, **pt.surface(arm))
        rx.sync()                                             # the loop-back runs on a handle of its own
        noise = dict(gain=math.sqrt(10 ** (pt.SNR_DB / 10)), noise_voltage=1.0, seed=pt.NOISE_SEED)
        chans = [dict(taps=(1.0,), **noise)] + [dict(taps=buf.ptr, n_taps=1, n_tap_sets=n, **noise) for buf in sets.values()]
        res = loopback(psdus, pt.ENC, pt.LEAD, slot, capi.EQ_LS, chans, psdu_stride=112)
    finally:
        for buf in sets.values():
            buf.free()
    good = {arm: int(((r["frames"]["flags"] & capi.F_CRC_OK) != 0).sum()) for arm, (r, _) in zip(pt.ARMS, res)}
    print("FCS-good of %d at %g dB per path: %r" % (n, pt.SNR_DB, good))
    assert good["direct"] == 0
    assert good["genie"] == n
    assert good["random"] < good["genie"]
    for arm, (r, x) in zip(pt.ARMS, res):
        assert_oracle_records(orc, r, x, slot, msg=arm, max_sym=n_sym)


# ---- 5. into the channel, and the stream block ----

def test_sets_feed_the_channel_on_the_device(rx):
    n_rows, row_len, N, L = 5, 200, 64, 8
    rng = np.random.default_rng(6)
    x = cnoise(rng, n_rows * row_len).reshape(n_rows, row_len)
    b2r, r2u, b2u = irs.los(8, [0.015, 0.015, 0], [0.12, 0.12, 4.5], [0.42, -0.08, 1.0])
    pdp = np.exp(-np.arange(L) / 2.0)
    d_taps, d_in, d_out = rx.alloc(n_rows * L * 8), rx.alloc(x.nbytes).upload(x), rx.alloc(x.nbytes)
    try:
        rx.irs_taps_dev(d_taps, n_rows, pdp / pdp.sum(), b2r, r2u, b2u, gain=1.0 / math.sqrt(N), k_factor=10.0, align_bits=2, seed=3)
        rx.channel_dev(d_in.ptr, d_out.ptr, x.size, n_rows, row_len=row_len, taps=d_taps.ptr, n_taps=L, n_tap_sets=n_rows,
                       cfo=np.float32(0.01))
        taps = d_taps.download(np.complex64, n_rows * L).reshape(n_rows, L)
        y = d_out.download(np.complex64, x.size).reshape(n_rows, row_len)
    finally:
        for buf in (d_taps, d_in, d_out):
            buf.free()
    assert np.isfinite(taps).all() and len(np.unique(taps)) == taps.size
    assert same(y, channel_ref.channel(x, taps=taps, cfo=np.float32(0.01)))


def test_block_with_a_surface(rx):
    cfg = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0), k_factor=5.0,
               pdp=(0.6, 0.3, 0.1), seed=11, refresh=1500)
    psi = irs.random_psi(16, 2, 4)
    n = 1000 + 4096 + 37 + 1000 + 37
    x = cnoise(np.random.default_rng(12), n)
    c = irs.IrsConfig(psi=psi, **cfg)
    sets = rx.irs_taps(n // 1500 + 1, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, k_factor=5.0, psi=psi, seed=11)
    # sample t runs through set t // refresh: the reference FIR with taps that switch on that sample
    coef = [(sets[np.arange(n) // 1500, l].real.copy(), sets[np.arange(n) // 1500, l].imag.copy()) for l in range(3)]
    want = channel_ref.mix(*channel_ref.fir(x, coef), inc=channel_ref.phase_inc(np.float32(2.0 * math.pi * 1e-3)), noise_voltage=0.0)
    outs = []
    for chunks in [(n,), (1000, 4096, 37, 1000, 37)]:
        blk = block.channel_model(noise_voltage=0.0, frequency_offset=1e-3, irs=irs.IrsConfig(psi=psi, **cfg))
        try:
            got, at = np.zeros(n, np.complex64), 0
            for m in chunks:
                assert blk.work([x[at:at + m]], [got[at:at + m]]) == m
                at += m
        finally:
            blk.close()
        outs.append(got)
    assert outs[0].tobytes() == outs[1].tobytes()
    assert same(outs[0], want)
    assert not same(outs[0][1500:1510], channel_ref.channel(x, taps=sets[0], cfo=np.float32(2.0 * math.pi * 1e-3))[1500:1510])
    # set_psi: from the next work() on the other configuration's taps
    blk = block.channel_model(noise_voltage=0.0, irs=irs.IrsConfig(psi=psi, **cfg))
    try:
        y = np.zeros(200, np.complex64)
        blk.work([x[:100]], [y[:100]])
        psi2 = irs.random_psi(16, 2, 5)
        blk.set_psi(psi2)
        blk.work([x[100:200]], [y[100:]])
        with pytest.raises(ValueError):
            blk.set_psi(np.ones(15))
    finally:
        blk.close()
    t2 = rx.irs_taps(1, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, k_factor=5.0, psi=psi2, seed=11)[0]
    assert same(y[:100], channel_ref.channel(x[:200], taps=sets[0])[:100]) and same(y[100:], channel_ref.channel(x[:200], taps=t2)[100:])
