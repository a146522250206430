"""wifirx_irs_taps_multi and wifirx_irs_sweep_multi, the reflecting surface behind an AP of M antennas (wr_irs.hip, wr_irs_sweep.hip, NUMERICS.md
rules 27 and 28), on the device:
  * given scatter: taps, elements, codes / powers, winners, taps value for value tests/irs_multi_ref.py, over 1 / 2 / 3 / 8 antennas,
    the lane tail and several passes of N, 1 / 3 / 16 taps, wrapped psi sets and scatter rows, Rayleigh and Rician, the direct path on
    and blocked, align_bits 1..3; for the sweep 3, 16, 15, 18 and 128 rows (one tile, a full tile, a spare row, two tiles, eight
    tiles), several sets per tile, the column tails of K; the caps N = 4096 with M = 8 and K = 1024;
  * without host arithmetic: M = 1 is wifirx_irs_taps / wifirx_irs_sweep byte for byte (Philox too), plane 0 of M = 4 is
    wifirx_irs_taps with the same seed, plane m is wifirx_irs_taps on the rows (w_a[m], w_b, w_d[m]), and with one tap the power
    is the float32 sum of the antennas' wifirx_irs_sweep powers;
  * Philox scatter: the chain exact on the device's own elements, the winner's planes within rule 26's bound of
    wifirx_irs_taps_multi(psi = codebook[best]), the same seed the same bytes, every antenna its own draws;
  * guard regions, outputs not asked for, refused arguments; the planes into wifirx_channel; the block with two ports;
  * one end-to-end point: a link that antenna 0 alone loses and the MRC of the antennas keeps."""
import json
import math
import os

import numpy as np
import pytest

import channel_ref
import irs_multi_ref as mr
import irs_sweep_ref as sr
from channel_helpers import cnoise, rx, same  # noqa: F401 (rx: fixture)
from wifirx import block, capi, irs, txgen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def scene(rng, M, N, L, n_scatter):
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    return crandn(rng, M, N), crandn(rng, N), crandn(rng, M), pdp, crandn(rng, n_scatter, (M + 1) * N + M)


def book(rng, K, N):
    """K unit-modulus configurations: even entries of any phase, odd entries on the 2-bit table (exact zeros in either part)"""
    cb = np.exp(1j * rng.uniform(-np.pi, np.pi, (K, N))).astype(np.complex64)
    cb[1::2] = irs.quantize(cb[1::2], 2)
    return cb


def sweep(rx, n_sets, pdp, a, b, d, cb, cb_dev=False, **kw):
    d_cb = rx.alloc(cb.nbytes).upload(cb) if cb_dev else None
    try:
        return rx.irs_sweep_multi(n_sets, pdp, a, b, d, codebook=d_cb if cb_dev else cb,
                                  **(dict(kw, n_codes=cb.shape[0]) if cb_dev else kw))
    finally:
        if d_cb is not None:
            d_cb.free()


# ---- 1. the cascade, given scatter, value for value ----

#             M  N    L   n_sets k_factor direct align_bits
TAPS_CASES = [(1, 1, 1, 1, 0.0, 1.0, 0),
              (2, 63, 3, 5, 10.0, 1.0, 0),
              (3, 64, 16, 1, 10.0, 0.0, 0),
              (8, 65, 3, 5, 0.0, 1.0, 0),
              (8, 130, 1, 5, 10.0, 1.0, 0),
              (2, 130, 16, 5, 0.0, 0.0, 0),
              (3, 65, 3, 5, 10.0, 1.0, 1),
              (8, 63, 1, 5, 10.0, 0.0, 2),
              (2, 64, 16, 1, 0.0, 1.0, 3),
              (1, 130, 3, 5, 10.0, 1.0, 2)]


@pytest.mark.parametrize("M,N,L,n_sets,k_factor,dg,bits", TAPS_CASES)
def test_taps_given_scatter_value_for_value(rx, M, N, L, n_sets, k_factor, dg, bits):
    rng = np.random.default_rng(10000 * M + 100 * L + N)
    n_scatter = max(1, n_sets * L - 2)                        # shorter than n_sets * L: the rows wrap
    a, b, d, pdp, sc = scene(rng, M, N, L, n_scatter)
    psi = None if bits else crandn(rng, 2, N)                 # two psi sets for up to five tap sets: they wrap
    kw = dict(gain=1.3, k_factor=k_factor, direct_gain=dg, scatter=sc, psi=psi, align_bits=bits)
    want = mr.irs_taps_multi(n_sets, pdp, a, b, d, **kw)
    got = rx.irs_taps_multi(n_sets, pdp, a, b, d if dg else None, want_elems=True, want_codes=bool(bits), **kw)
    assert got["taps"].shape == (M, n_sets, L) and same(got["taps"], want["taps"])
    assert same(got["elems"], want["elems"])
    if bits:
        assert np.array_equal(got["codes"], want["codes"]) and (got["codes"] < (1 << bits)).all()
    assert np.isfinite(got["taps"]).all()
    if N > 1:                                                 # (sets that wrap onto one scatter row and one psi set repeat)
        assert np.unique(got["taps"][:, 0]).size == M * L


def test_taps_at_the_caps(rx):
    M, N, L, n_sets = 8, 4096, 1, 2
    rng = np.random.default_rng(8)
    a, b, d, pdp, sc = scene(rng, M, N, L, 2)
    kw = dict(k_factor=10.0, scatter=sc, psi=crandn(rng, N), gain=1.0 / 64)
    want = mr.irs_taps_multi(n_sets, pdp, a, b, d, **kw)
    got = rx.irs_taps_multi(n_sets, pdp, a, b, d, want_elems=True, **kw)
    assert same(got["taps"], want["taps"]) and same(got["elems"], want["elems"])


# ---- 2. the cascade against wifirx_irs_taps, no host arithmetic ----

def test_taps_against_the_single_antenna_call(rx):
    N, L, n_sets = 130, 3, 5
    rng = np.random.default_rng(21)
    a, b, d, pdp, sc = scene(rng, 4, N, L, 7)
    psi = crandn(rng, 2, N)
    for kw in (dict(psi=psi), dict(align_bits=2)):
        kw = dict(kw, k_factor=3.0, gain=0.7, want_elems=True, want_codes="align_bits" in kw)
        # one antenna is that call, byte for byte, with given and with Philox scatter
        for src in (dict(seed=77), dict(scatter=mr.antenna_rows(sc, 4, N, 0))):
            one = rx.irs_taps_multi(n_sets, pdp, a[:1], b, d[:1], **src, **kw)
            old = rx.irs_taps(n_sets, pdp, a[0], b, d[0], **src, **kw)
            assert one["taps"][0].tobytes() == old["taps"].tobytes() and one["elems"].tobytes() == old["elems"].tobytes()
            if kw["want_codes"]:
                assert one["codes"].tobytes() == old["codes"].tobytes()
        # plane 0 of four antennas with Philox scatter is that call with the same seed
        four = rx.irs_taps_multi(n_sets, pdp, a, b, d, seed=77, **kw)
        old = rx.irs_taps(n_sets, pdp, a[0], b, d[0], seed=77, **kw)
        assert four["taps"][0].tobytes() == old["taps"].tobytes()
        assert four["elems"][:, :, 0].tobytes() == old["elems"][:, :, 0].tobytes()
        assert four["elems"][:, :, 4].tobytes() == old["elems"][:, :, 1].tobytes()
    # given scatter and given phases: plane m is that call on the rows (w_a[m], w_b, w_d[m])
    four = rx.irs_taps_multi(n_sets, pdp, a, b, d, scatter=sc, psi=psi, k_factor=3.0)
    for m in range(4):
        old = rx.irs_taps(n_sets, pdp, a[m], b, d[m], scatter=mr.antenna_rows(sc, 4, N, m), psi=psi, k_factor=3.0)
        assert four[m].tobytes() == old.tobytes(), m


# ---- 3. the sweep, given scatter, value for value ----

#              M  L   n_sets N    K     k_factor direct cb_dev
SWEEP_CASES = [(1, 3, 7, 63, 15, 10.0, 1.0, False),          # 3 rows: five sets per tile, a ragged last tile
               (2, 8, 3, 64, 16, 0.0, 1.0, True),            # 16 rows: an exactly full tile
               (3, 5, 3, 65, 17, 10.0, 0.0, False),          # 15 rows: a tile with a spare row
               (3, 6, 3, 130, 100, 10.0, 1.0, False),        # 18 rows: two tiles
               (3, 6, 1, 1, 1, 0.0, 1.0, False),
               (8, 16, 2, 3, 17, 10.0, 1.0, True),           # 128 rows: eight tiles
               (8, 16, 1, 65, 16, 0.0, 0.0, False),
               (2, 2, 7, 1, 16, 10.0, 1.0, False),           # 4 rows: four sets per tile, 7 sets
               (2, 2, 7, 64, 100, 0.0, 1.0, True),
               (2, 1, 3, 3, 1024, 10.0, 1.0, True),          # the cap of K
               (5, 4, 2, 63, 1024, 10.0, 1.0, False)]        # 20 rows at the cap of K: the running powers of 16 groups


@pytest.mark.parametrize("M,L,n_sets,N,K,k_factor,dg,cb_dev", SWEEP_CASES)
def test_sweep_given_scatter_value_for_value(rx, M, L, n_sets, N, K, k_factor, dg, cb_dev):
    rng = np.random.default_rng(100000 * M + 1000 * L + N + K)
    n_scatter = max(1, n_sets * L - 2)
    a, b, d, pdp, sc = scene(rng, M, N, L, n_scatter)
    cb = book(rng, K, N)
    kw = dict(gain=1.3, k_factor=k_factor, direct_gain=dg, scatter=sc)
    want = mr.irs_sweep_multi(n_sets, pdp, a, b, d, codebook=cb, **kw)
    got = sweep(rx, n_sets, pdp, a, b, d if dg else None, cb, cb_dev, **kw)
    assert same(got["power"], want["power"])
    assert np.array_equal(got["best"], want["best"]) and got["best"].dtype == np.uint16
    assert got["taps"].shape == (M, n_sets, L) and same(got["taps"], want["taps"])
    if N >= 63:
        assert np.unique(got["power"][0]).size == K           # the entries differ


def test_sweep_ties_and_nan_over_two_tiles(rx):
    M, N, L, n_sets = 3, 65, 6, 3
    rng = np.random.default_rng(2)
    a, b, d, pdp, sc = scene(rng, M, N, L, n_sets * L)
    kw = dict(k_factor=3.0, scatter=sc)
    two = book(rng, 2, N)
    cb = np.stack([two[0], two[1], two[1], two[0]])           # entries 0 = 3 and 1 = 2: the lower one wins
    got, want = sweep(rx, n_sets, pdp, a, b, d, cb, **kw), mr.irs_sweep_multi(n_sets, pdp, a, b, d, codebook=cb, **kw)
    assert same(got["power"], want["power"]) and same(got["power"][:, 0], got["power"][:, 3])
    assert np.array_equal(got["best"], want["best"]) and (got["best"] < 2).all() and same(got["taps"], want["taps"])
    for at in (0, 2):                                         # an entry holding a NaN never wins
        cb = np.stack([two[0], two[1], two[0]])
        cb[at, N // 2] = np.nan
        got, want = sweep(rx, n_sets, pdp, a, b, d, cb, **kw), mr.irs_sweep_multi(n_sets, pdp, a, b, d, codebook=cb, **kw)
        assert np.isnan(got["power"][:, at]).all() and np.array_equal(np.isnan(got["power"]), np.isnan(want["power"]))
        assert np.array_equal(got["best"], want["best"]) and (got["best"] != at).all() and same(got["taps"], want["taps"])
    cb = np.stack([two[0], two[1], two[0]])                   # all NaN: the winner is 0
    cb[:, 5] = np.nan
    got = sweep(rx, n_sets, pdp, a, b, d, cb, **kw)
    assert np.isnan(got["power"]).all() and (got["best"] == 0).all() and np.isnan(got["taps"]).all()


# ---- 4. the sweep against wifirx_irs_sweep, no host arithmetic ----

def test_sweep_against_the_single_antenna_call(rx):
    N, L, n_sets, K = 130, 3, 7, 100
    rng = np.random.default_rng(41)
    a, b, d, pdp, sc = scene(rng, 3, N, L, 5)
    cb = book(rng, K, N)
    for src in (dict(seed=0x1234567890), dict(scatter=mr.antenna_rows(sc, 3, N, 0))):
        one = sweep(rx, n_sets, pdp, a[:1], b, d[:1], cb, k_factor=3.0, **src)
        old = rx.irs_sweep(n_sets, pdp, a[0], b, d[0], codebook=cb, k_factor=3.0, **src)
        assert one["taps"][0].tobytes() == old["taps"].tobytes() and one["best"].tobytes() == old["best"].tobytes()
        assert one["power"].tobytes() == old["power"].tobytes()
    # one tap: the metric is the float32 sum, in ascending m, of the antennas' own powers
    many = sweep(rx, n_sets, pdp[:1], a, b, d, cb, k_factor=3.0, scatter=sc)
    singles = [rx.irs_sweep(n_sets, pdp[:1], a[m], b, d[m], codebook=cb, k_factor=3.0, scatter=mr.antenna_rows(sc, 3, N, m))["power"]
               for m in range(3)]
    assert same(many["power"], (singles[0] + singles[1]) + singles[2])
    assert not np.array_equal(many["best"], sr.winner(singles[0])) or not np.array_equal(many["best"], sr.winner(singles[1]))


# ---- 5. Philox scatter ----

@pytest.mark.parametrize("M,N,L,n_sets,K", [(4, 65, 3, 5, 17), (3, 130, 6, 3, 100), (8, 64, 1, 5, 16)])
def test_philox_scatter(rx, M, N, L, n_sets, K):
    rng = np.random.default_rng(N + M)
    a, b, d, pdp, _ = scene(rng, M, N, L, 1)
    cb = book(rng, K, N)
    seed = 0xFEDCBA9876543210
    scale = np.sqrt(pdp.astype(np.float64)).astype(np.float32)
    psi = crandn(rng, N)
    for k_factor in (0.0, 10.0):
        # the direct path is blocked (it would be one more draw through the device's own Box-Muller); the device's elements
        # go into the restatement, and the rest of both chains is exact
        kw = dict(k_factor=k_factor, direct_gain=0.0, seed=seed)
        casc = rx.irs_taps_multi(n_sets, pdp, a, b, None, psi=psi, want_elems=True, **kw)
        again = rx.irs_taps_multi(n_sets, pdp, a, b, None, psi=psi, want_elems=True, **kw)
        el = casc["elems"]
        assert casc["taps"].tobytes() == again["taps"].tobytes() and el.tobytes() == again["elems"].tobytes()
        assert same(casc["taps"], mr.irs_taps_multi(n_sets, pdp, a, b, None, psi=psi, elems=el, **kw)["taps"])
        for bits in (1, 3):
            ga = rx.irs_taps_multi(n_sets, pdp, a, b, None, align_bits=bits, want_elems=True, want_codes=True, **kw)
            wa = mr.irs_taps_multi(n_sets, pdp, a, b, None, align_bits=bits, elems=el, **kw)
            assert same(ga["elems"], el) and np.array_equal(ga["codes"], wa["codes"]) and same(ga["taps"], wa["taps"])
        if k_factor == 0.0:                                   # every (antenna, r, l, n) and the shared leg: draws of their own
            assert np.unique(el).size == el.size and abs(float((np.abs(el) ** 2).mean()) - 1.0) < 0.05
        # the host's Philox and Box-Muller give the same elements to rule 17's 1e-5 (the counters are the rule's)
        host = mr.irs_taps_multi(n_sets, pdp, a, b, None, psi=psi, **kw)["elems"]
        assert float(np.abs(el - host).max()) <= 1e-5
        got = sweep(rx, n_sets, pdp, a, b, None, cb, **kw)
        want = mr.irs_sweep_multi(n_sets, pdp, a, b, None, codebook=cb, elems=el, **kw)
        assert same(got["power"], want["power"]) and np.array_equal(got["best"], want["best"]) and same(got["taps"], want["taps"])
        assert sweep(rx, n_sets, pdp, a, b, None, cb, **kw)["taps"].tobytes() == got["taps"].tobytes()
        # rule 27 with the winner's configuration: the same value rounded in another order, within rule 26's bound per antenna
        other = rx.irs_taps_multi(n_sets, pdp, a, b, None, psi=cb[got["best"]], **kw)
        worst = 0.0
        for m in range(M):
            lim = sr.bound(np.zeros((n_sets, L)), el[:, :, m, :], el[:, :, M, :], scale)
            err = np.abs(got["taps"][m].astype(np.complex128) - other[m].astype(np.complex128))
            worst = max(worst, float((err / lim).max()))
            assert (err <= lim).all(), m
        print("M = %d, N = %d, K = %g: winner's planes against wifirx_irs_taps_multi, largest error / bound = %.4f"
              % (M, N, k_factor, worst))
    # with the direct path: one more Box-Muller sample of at most unit scale (1e-5) times a tap scale of at most 1, and the
    # one rounding of h_d + sum that it may move
    kw = dict(k_factor=10.0, seed=seed, psi=psi)
    full = rx.irs_taps_multi(n_sets, pdp, a, b, d, want_elems=True, **kw)
    rest = mr.irs_taps_multi(n_sets, pdp, a, b, d, elems=full["elems"], **kw)
    assert float(np.abs(full["taps"] - rest["taps"]).max()) <= 1e-5 + 2.0 ** -23 * float(np.abs(rest["taps"]).max())
    assert np.unique(full["taps"] - rx.irs_taps_multi(n_sets, pdp, a, b, None, direct_gain=0.0, **kw)).size == M * n_sets * L


# ---- 6. guard regions, outputs that were not asked for, refused arguments ----

def test_nothing_beyond_what_was_asked_for(rx):
    M, N, L, n_sets, K, guard = 3, 65, 6, 5, 17, 64
    rng = np.random.default_rng(4)
    a, b, d, pdp, _ = scene(rng, M, N, L, 1)
    cb = book(rng, K, N)
    filled = lambda v: rx.alloc(v + guard).upload(np.full(v + guard, 0xA5, np.uint8))
    sizes = {"taps": M * n_sets * L * 8, "elems": n_sets * L * (M + 1) * N * 8, "codes": n_sets * N}
    for bits, want in [(0, ()), (2, ()), (2, ("codes",)), (0, ("elems",)), (2, ("elems", "codes"))]:
        bufs = {k: filled(v) for k, v in sizes.items()}
        rx.irs_taps_multi_dev(bufs["taps"], n_sets, pdp, a, b, d, k_factor=3.0, psi=None if bits else irs.random_psi(N, 2, 1),
                              align_bits=bits, seed=9, elems_ptr=bufs["elems"] if "elems" in want else None,
                              codes_ptr=bufs["codes"] if "codes" in want else None)
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
    for Ls in (2, 6):                                         # 6 rows (one tile, two sets in it) and 18 rows (two tiles)
        sizes = {"taps": M * n_sets * Ls * 8, "best": n_sets * 2, "power": n_sets * K * 4}
        full = None
        for leave in (None, "taps", "best", "power"):
            bufs = {k: filled(v) for k, v in sizes.items()}
            ptr = {k: (None if k == leave else bufs[k]) for k in sizes}
            rx.irs_sweep_multi_dev(ptr["taps"], n_sets, pdp[:Ls], a, b, d, codebook=cb, k_factor=3.0, seed=9, best_ptr=ptr["best"],
                                   power_ptr=ptr["power"])
            got = {k: bufs[k].download(np.uint8, v + guard) for k, v in sizes.items()}
            for buf in bufs.values():
                buf.free()
            if leave is None:
                full = got
            for k, v in sizes.items():
                assert (got[k][v:] == 0xA5).all(), (Ls, leave, k, "the guard region")
                if k == leave:
                    assert (got[k][:v] == 0xA5).all(), (Ls, leave, "written without being asked for")
                else:
                    assert got[k][:v].tobytes() == full[k][:v].tobytes(), (Ls, leave, k, "depends on which outputs are asked for")
        assert np.isfinite(full["taps"][:sizes["taps"]].view(np.complex64)).all()
        assert (full["best"][:sizes["best"]].view(np.uint16) < K).all()


def test_refused_arguments_write_nothing():
    import ctypes as C
    rx = capi.WifiRx(max_sym=1, device=0)
    try:
        lib, M, N, L, K, n_sets = capi.lib(), 2, 8, 2, 5, 3
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        words = M * n_sets * L * 2 + n_sets * K + n_sets + 16
        out = rx.alloc(words * 4).upload(np.full(words, 0x7FC0DEAD, np.uint32))
        canary = out.download(np.uint8, words * 4)
        taps_p, power_p = out.ptr, out.ptr + M * n_sets * L * 8
        best_p = power_p + n_sets * K * 4
        dev = rx.alloc(4096)                     # stands for device psi, codebook, scatter, elems and codes
        arr = dict(pdp=np.array([1.0, 0.5], np.float32), a=np.ones((M, N), np.complex64), b=np.ones(N, np.complex64),
                   d=np.ones(M, np.complex64), cb=np.ones((K, N), np.complex64), psi=np.ones(N, np.complex64))
        keep = []

        def pdp(*v):
            keep.append(np.array(v, np.float32))
            return P(keep[-1])

        def shared(v):
            return (v["taps"], v["n_ant"], v["n_sets"], v["n_taps"], v["pdp"], v["gain"], v["n_elems"], v["a"], v["b"], v["d"],
                    v["k"], v["dg"])

        def taps(**kw):
            v = dict(taps=taps_p, n_ant=M, n_sets=n_sets, n_taps=L, pdp=P(arr["pdp"]), gain=1.0, n_elems=N, a=P(arr["a"]),
                     b=P(arr["b"]), d=P(arr["d"]), k=1.0, dg=1.0, psi=P(arr["psi"]), psi_dev=0, n_psi=1, bits=0, scatter=None,
                     n_scatter=0, seed=1, elems=None, codes=None)
            v.update(kw)
            return lib.wifirx_irs_taps_multi(rx._h, *shared(v), v["psi"], v["psi_dev"], v["n_psi"], v["bits"], v["scatter"],
                                             v["n_scatter"], v["seed"], v["elems"], v["codes"])

        def swp(**kw):
            v = dict(taps=taps_p, n_ant=M, n_sets=n_sets, n_taps=L, pdp=P(arr["pdp"]), gain=1.0, n_elems=N, a=P(arr["a"]),
                     b=P(arr["b"]), d=P(arr["d"]), k=1.0, dg=1.0, cb=P(arr["cb"]), cb_dev=0, n_codes=K, scatter=None, n_scatter=0,
                     seed=1, best=best_p, power=power_p)
            v.update(kw)
            return lib.wifirx_irs_sweep_multi(rx._h, *shared(v), v["cb"], v["cb_dev"], v["n_codes"], v["scatter"], v["n_scatter"],
                                              v["seed"], v["best"], v["power"])

        inf, nan = float("inf"), float("nan")
        both = [dict(n_ant=0), dict(n_ant=9),
                dict(pdp=None), dict(a=None), dict(b=None), dict(d=None), dict(scatter=dev.ptr, n_scatter=0),
                dict(n_elems=0), dict(n_elems=4097), dict(n_taps=0), dict(n_taps=17, pdp=pdp(*([1.0] * 17))),
                dict(k=-1.0), dict(k=nan), dict(k=inf),
                dict(pdp=pdp(1.0, -0.5)), dict(pdp=pdp(nan, 1.0)), dict(pdp=pdp(1.0, inf)),
                dict(gain=nan), dict(gain=inf), dict(dg=nan), dict(dg=-inf),
                dict(scatter=dev.ptr + 4, n_scatter=1), dict(pdp=P(arr["pdp"]).value + 1), dict(taps=taps_p + 4),
                dict(a=P(arr["a"]).value + 2), dict(b=P(arr["b"]).value + 1), dict(d=P(arr["d"]).value + 2)]
        for kw in both:
            assert taps(**kw) == capi.EINVAL, kw
            assert swp(**kw) == capi.EINVAL, kw
        for kw in [dict(taps=None), dict(bits=4), dict(psi=None), dict(n_psi=0), dict(codes=dev.ptr), dict(elems=dev.ptr + 4),
                   dict(psi=dev.ptr + 4, psi_dev=1), dict(psi=P(arr["psi"]).value + 2)]:
            assert taps(**kw) == capi.EINVAL, kw
        for kw in [dict(cb=None), dict(n_codes=0), dict(n_codes=1025), dict(taps=None, best=None, power=None),
                   dict(power=power_p + 2), dict(best=best_p + 1), dict(cb=dev.ptr + 4, cb_dev=1), dict(cb=P(arr["cb"]).value + 2)]:
            assert swp(**kw) == capi.EINVAL, kw
        # every check comes before n_sets = 0 is looked at; n_sets = 0 itself does nothing; too many sets are out of range
        assert taps(n_sets=0, n_ant=9) == capi.EINVAL and swp(n_sets=0, n_ant=0) == capi.EINVAL
        assert taps(n_sets=0) == capi.OK and swp(n_sets=0) == capi.OK
        assert taps(n_sets=1 << 31) == capi.ERANGE and swp(n_sets=1 << 31) == capi.ERANGE
        rx.sync()
        assert out.download(np.uint8, words * 4).tobytes() == canary.tobytes(), "a refused call wrote"
        # what the checks let through
        assert taps(d=None, dg=0.0) == capi.OK and taps(bits=2, psi=None, n_psi=0, codes=dev.ptr) == capi.OK
        assert swp(best=None, power=None) == capi.OK and swp(taps=None, best=None, d=None, dg=0.0) == capi.OK
        assert taps(n_ant=8, n_sets=0) == capi.OK and swp(n_ant=1) == capi.OK
        rx.sync()
        assert np.isfinite(out.download(np.complex64, M * n_sets * L)).all()
        out.free()
        dev.free()
    finally:
        rx.close()


# ---- 7. into the channel, and the stream block ----

def test_planes_feed_the_channel_on_the_device(rx):
    M, n_rows, row_len, S, L = 3, 5, 200, 8, 8
    rng = np.random.default_rng(6)
    x = cnoise(rng, n_rows * row_len).reshape(n_rows, row_len)
    b2r, r2u, b2u = irs.los(S, [0.015, 0.015, 0], [0.12, 0.12, 4.5], [0.42, -0.08, 1.0], antennas=M)
    cb = irs.dft_codebook(S, b2r[0], over=1, bits=2)
    pdp = np.exp(-np.arange(L) / 2.0)
    d_taps, d_in, d_out = rx.alloc(M * n_rows * L * 8), rx.alloc(x.nbytes).upload(x), rx.alloc(x.nbytes)
    try:
        rx.irs_sweep_multi_dev(d_taps, n_rows, pdp / pdp.sum(), b2r, r2u, b2u, codebook=cb, gain=1.0 / S, k_factor=10.0, seed=3)
        taps = d_taps.download(np.complex64, M * n_rows * L).reshape(M, n_rows, L)
        assert np.isfinite(taps).all() and len(np.unique(taps)) == taps.size
        for m in range(M):
            rx.channel_dev(d_in.ptr, d_out.ptr, x.size, n_rows, row_len=row_len, taps=d_taps.ptr + m * n_rows * L * 8, n_taps=L,
                           n_tap_sets=n_rows, cfo=np.float32(0.01))
            y = d_out.download(np.complex64, x.size).reshape(n_rows, row_len)
            assert same(y, channel_ref.channel(x, taps=taps[m], cfo=np.float32(0.01))), m
    finally:
        for buf in (d_taps, d_in, d_out):
            buf.free()


@pytest.mark.parametrize("trained", [False, True])
def test_block_with_two_ports(rx, trained):
    cfg = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0), k_factor=5.0,
               pdp=(0.6, 0.3, 0.1), seed=11, refresh=1500, antennas=2)
    how = dict(codebook=irs.dft_codebook(4, over=2, bits=2)) if trained else dict(psi=irs.random_psi(16, 2, 4))
    n = 1000 + 4096 + 37
    x = cnoise(np.random.default_rng(12), n)
    c = irs.IrsConfig(**how, **cfg)
    assert c.los_b2r.shape == (2, 16) and c.los_b2u.shape == (2,)
    kw = dict(k_factor=5.0, seed=11)
    if trained:
        direct = rx.irs_sweep_multi(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, codebook=c.codebook, **kw)
        sets = direct["taps"]
    else:
        sets = rx.irs_taps_multi(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, psi=c.psi, **kw)
    inc = channel_ref.phase_inc(np.float32(2.0 * math.pi * 1e-3))
    want = []
    for m in range(2):       # sample t runs through set t // refresh of plane m: the reference FIR with taps that switch there
        coef = [(sets[m, np.arange(n) // 1500, l].real.copy(), sets[m, np.arange(n) // 1500, l].imag.copy()) for l in range(3)]
        want.append(channel_ref.mix(*channel_ref.fir(x, coef), inc=inc, noise_voltage=0.0))
    outs = []
    for chunks in [(n,), (1000, 4096, 37)]:
        blk = block.channel_model(noise_voltage=0.0, frequency_offset=1e-3, irs=irs.IrsConfig(**how, **cfg))
        try:
            assert len(blk.out_sig) == 2 and len(blk.in_sig) == 1
            got, at = np.zeros((2, n), np.complex64), 0
            for m in chunks:
                assert blk.work([x[at:at + m]], [got[0, at:at + m], got[1, at:at + m]]) == m
                at += m
            if trained:
                best = blk.irs_best
                assert np.array_equal(best[:16], direct["best"][:best.size][:16])
            else:
                blk.set_psi(irs.random_psi(16, 2, 5))
        finally:
            blk.close()
        outs.append(got)
    assert outs[0].tobytes() == outs[1].tobytes()
    assert same(outs[0][0], want[0]) and same(outs[0][1], want[1]) and not same(outs[0][0], outs[0][1])
    # the ports' noise: port m draws from noise_seed + m
    blk = block.channel_model(noise_voltage=0.5, noise_seed=40, irs=irs.IrsConfig(**how, **cfg))
    try:
        y = np.zeros((2, 300), np.complex64)
        blk.work([x[:300]], [y[0], y[1]])
    finally:
        blk.close()
    for m in range(2):
        assert y[m].tobytes() == rx.channel(x[:300], taps=sets[m, 0], noise_voltage=0.5, seed=40 + m).tobytes(), m
    clean = [rx.channel(x[:300], taps=sets[m, 0]) for m in range(2)]
    assert not same(y[0] - clean[0], y[1] - clean[1])        # two noise sequences


# ---- 8. one end-to-end point (tests/irs_multi_point.py looked for it on the host) ----

def test_antennas_close_a_link_one_antenna_cannot():
    """256 QPSK-1/2 frames behind a 64-element 2-bit surface trained on the MRC metric, eight taps, the batch chain on the device:
    tx_batch -> irs_sweep_multi -> one channel per antenna on its plane, each with its own noise seed -> demod ->
    diversity_combine (MRC) -> decode_mac -> link_stats.  At the point tests/irs_multi_point.py found on the host chain (A = 4,
    -23 dB per path and antenna: 14 and 249 of 256, and the same two inequalities hold at -24 and -22 dB; A = 2 has no such
    point; profiles/irs_multi_operating_point.json) antenna 0 alone decodes at most a quarter of the frames and the MRC at
    least three quarters."""
    import irs_multi_point as pt
    with open(os.path.join(ROOT, "profiles", "irs_multi_operating_point.json")) as f:
        rec = json.load(f)
    point = [p for p in rec["points"] if p["snr_db"] == rec["chosen_snr_db"]][0]
    assert rec["chosen_snr_db"] == pt.SNR_DB and rec["chosen_antennas"] == pt.N_ANT == point["antennas"] and point["holds"]
    assert rec["neighbours_hold"] and len(rec["points"]) == 3
    for p in rec["points"]:                                   # the point and 1 dB to either side, on the host chain
        assert p["single"] <= pt.SINGLE_AT_MOST and p["mrc"] >= pt.MRC_AT_LEAST, p
    n, A, L = pt.N_FRAMES, pt.N_ANT, pt.N_TAPS
    n_sym, slot = pt.geometry()
    b2r, r2u = pt.scene()
    rx = capi.WifiRx(max_sym=n_sym, llr_bits=2, want_carrier=True, device=0)
    bufs = []
    try:
        psdus = txgen.make_psdus(n, pt.PLEN, seed=pt.PSDU_SEED)
        d_psdu = rx.alloc(n * pt.PLEN).upload(psdus)
        tx, iq, taps, d_best = rx.alloc(n * slot * 8), rx.alloc(n * slot * 8), rx.alloc(A * n * L * 8), rx.alloc(n * 2)
        bufs += [d_psdu, tx, iq, taps, d_best]
        rx.tx_batch_dev(tx.ptr, n * slot, d_psdu.ptr, pt.ENC, psdu_len=np.full(n, pt.PLEN, np.uint32), psdu_stride=pt.PLEN, lead=pt.LEAD,
                        row_len=slot)
        ref = rx.alloc_out(n)
        rx.demod_batch_dev(tx.ptr, slot, n, ref)
        ref["psdu"], ref["psdu_stride"] = d_psdu, pt.PLEN
        assert rx.link_stats(n, ref, ref)["frames_ref"] == n
        rx.irs_sweep_multi_dev(taps, n, pt.PDP, b2r, r2u, None, best_ptr=d_best, **pt.surface())
        ins = []
        for m in range(A):
            rx.channel_dev(tx.ptr, iq.ptr, n * slot, n, row_len=slot, taps=taps.ptr + m * n * L * 8, n_taps=L, n_tap_sets=n,
                           gain=math.sqrt(10 ** (pt.SNR_DB / 10)), noise_voltage=1.0, seed=pt.NOISE_SEED + m)
            ins.append(rx.alloc_out(n, psdu_stride=112, want_csi=True))
            rx.demod_batch_dev(iq.ptr, slot, n, ins[m])
        out = rx.alloc_out(n, psdu_stride=112)
        rx.diversity_combine_dev(ins, n, out, capi.DIV_MRC)
        good, wrong = {}, 0
        for name, dev in (("single", ins[0]), ("mrc", out)):
            rx.decode_batch_dev(n, dev)
            r = rx.link_stats(n, dev, ref)
            good[name], wrong = r["frames_psdu_ok"], wrong + r["frames_crc_ok_wrong"]
        best = d_best.download(np.uint16, n)
        for d in ins + [out]:
            rx.free_out(d)
        rx.free_out(ref)
    finally:
        for b in bufs:
            b.free()
        rx.close()
    print("FCS-good of %d at %g dB per path and antenna, A = %d: %r (host chain: single %d, mrc %d); %d distinct winners"
          % (n, pt.SNR_DB, A, good, point["single"], point["mrc"], np.unique(best).size))
    # the device's elements differ from the host's in the last bits of the Box-Muller (rule 17's 1e-5), so a frame on the edge
    # may fall the other way: the counts are held to the two inequalities, not to the host's exact numbers
    assert wrong == 0
    assert good["single"] <= pt.SINGLE_AT_MOST
    assert good["mrc"] >= pt.MRC_AT_LEAST
