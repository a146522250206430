"""wifirx_irs_estimate, the surface configured from noisy pilot observations (wr_irs_estimate.hip, NUMERICS.md rule 29), on the device:
  * given scatter and given noise: observations, estimate, codes and taps value for value tests/irs_estimate_ref.py, over the
    shapes at which the tiles can go wrong (N 3 / 16 grouped / 65, T 1 / 5 / 17 / 65 / 1024, J 15 / 16 / 17 / 1024, R 1 / 3 with
    7 sets / 16 / 18 / 128), every subset of the outputs, sentinels behind and in what was not asked for;
  * kernel against kernel, no host arithmetic beyond rule 28's power sum: the observations against wifirx_irs_sweep_multi's powers on
    the group-expanded pilots, the taps against wifirx_irs_taps_multi / wifirx_irs_taps on the phases of the decided codes;
  * Philox scatter and noise: exact on the device's own elements, the drawn noise within 1e-5 of the host's;
  * estimate -> wifirx_channel queued without a sync;
  * end to end at tests/irs_estimate_point.py's operating point: between the random surface and the genie."""
import json
import math
import os

import numpy as np
import pytest

import channel_ref
import irs_estimate_ref as er
import irs_multi_ref as mr
from channel_helpers import cnoise, rx, same  # noqa: F401 (rx: fixture)
from wifirx import block, capi, irs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def scene(rng, M, N, L, n_scatter):
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    return crandn(rng, M, N), crandn(rng, N), crandn(rng, M), pdp, crandn(rng, n_scatter, (M + 1) * N + M)


def any_pilots(rng, T, G):
    """T configurations of G groups: even slots of any phase and a modulus up to 1, odd slots on the 2-bit table (exact zeros in
    either part)"""
    pl = (rng.uniform(0.5, 1.0, (T, G)) * np.exp(1j * rng.uniform(-np.pi, np.pi, (T, G)))).astype(np.complex64)
    pl[1::2] = irs.quantize(pl[1::2], 2)
    return pl


def any_groups(rng, N, G):
    """a map of N elements onto G groups that uses every group"""
    g = np.concatenate([np.arange(G), rng.integers(0, G, N - G)]).astype(np.uint16)
    return rng.permutation(g)


def compare(got, want, bits):
    assert same(got["obs"], want["obs"]), "obs"
    assert same(got["est"], want["est"]), "est"
    if bits:
        assert np.array_equal(got["codes"], want["codes"]) and (got["codes"] < (1 << bits)).all(), "codes"
        assert same(got["taps"], want["taps"]), "taps"


# ---- 1. given scatter and given noise, value for value ----

#        M  L   n_sets N     G     T     k_factor direct sigma bits pilots
CASES = [(1, 1, 1, 3, 3, 1, 0.0, 1.0, 0.5, 2, "any"),            # one row, one pilot: 2 T = 2, two zero terms
         (1, 3, 7, 3, 3, 5, 10.0, 1.0, 0.5, 1, "any"),           # 3 rows, 7 sets: 21 rows in two tiles, sets across the border
         (1, 16, 2, 16, 4, 17, 0.0, 0.0, 1.0, 3, "any"),         # 16 rows: a set per tile; groups(4, 2); T past one column group
         (2, 9, 3, 65, 14, 65, 10.0, 1.0, 0.5, 2, "any"),        # 18 rows; N and T past a chunk by one; J = 15
         (8, 16, 2, 65, 15, 16, 3.0, 1.0, 0.25, 2, "hadamard"),  # 128 rows: eight tiles per set; J = 16, T = 16
         (2, 1, 5, 65, 16, 17, 0.0, 1.0, 2.0, 3, "dft"),         # J = 17: a second column group of one column
         (8, 3, 2, 16, 16, 32, 0.0, 0.0, 0.0, 2, "hadamard"),    # 24 rows; sigma = 0: obs = x; direct path blocked
         (2, 3, 1, 3, 3, 1024, 10.0, 1.0, 0.5, 1, "any"),        # the cap of T
         (1, 1, 1, 1023, 1023, 5, 0.0, 1.0, 0.5, 2, "any"),      # the cap of J
         (1, 1, 3, 1, 1, 1, 0.0, 1.0, 0.0, 1, "any")]


def make_case(M, L, n_sets, N, G, T, k_factor, dg, sigma, bits, kind):
    rng = np.random.default_rng(100000 * M + 1000 * L + N + G + T)
    a, b, d, pdp, sc = scene(rng, M, N, L, max(1, n_sets * L - 2))       # shorter than n_sets * L: the rows wrap
    if kind == "any":
        pl = any_pilots(rng, T, G)
    else:
        pl = irs.dft_pilots(G) if kind == "dft" else irs.hadamard_pilots(G)
        assert pl.shape[0] == T
    gm = None if G == N else (irs.groups(4, 2) if (N, G) == (16, 4) else any_groups(rng, N, G))
    w = crandn(rng, max(1, n_sets * M * L - 1), T)                        # one row short: the noise rows wrap
    kw = dict(pilots=pl, group=gm, sigma=sigma, est_scale=np.float32(0.9 / T), align_bits=bits, gain=1.3, k_factor=k_factor,
              direct_gain=dg, scatter=sc, noise=w)
    return (n_sets, pdp, a, b, d if dg else None), (n_sets, pdp, a, b, d), kw


@pytest.mark.parametrize("M,L,n_sets,N,G,T,k_factor,dg,sigma,bits,kind", CASES)
def test_given_scatter_and_noise_value_for_value(rx, M, L, n_sets, N, G, T, k_factor, dg, sigma, bits, kind):
    dev_args, host_args, kw = make_case(M, L, n_sets, N, G, T, k_factor, dg, sigma, bits, kind)
    want = er.irs_estimate(*host_args, **kw)
    got = rx.irs_estimate(*dev_args, **kw)
    assert got["obs"].shape == (n_sets, M * L, T) and got["est"].shape == (n_sets, M * L, G + 1)
    assert got["codes"].shape == (n_sets, G) and got["taps"].shape == (M, n_sets, L)
    compare(got, want, bits)
    if sigma == 0:
        assert same(got["obs"], want["x"])
    # the same call again, and device copies of the pilots, the scatter and the noise, give the same bytes
    d_pl = rx.alloc(kw["pilots"].nbytes).upload(kw["pilots"])
    try:
        again = rx.irs_estimate(*dev_args, **kw)
        bufs = {k: rx.alloc(v.nbytes) for k, v in got.items()}
        d_sc = rx.alloc(kw["scatter"].nbytes).upload(kw["scatter"])
        d_w = rx.alloc(kw["noise"].nbytes).upload(kw["noise"])
        rx.irs_estimate_dev(bufs["taps"], *dev_args, **dict(kw, pilots=d_pl, n_pilots=T, n_groups=G, scatter=d_sc,
                                                           n_scatter=kw["scatter"].shape[0], noise=d_w, n_noise=kw["noise"].shape[0]),
                            est_ptr=bufs["est"], codes_ptr=bufs["codes"], obs_ptr=bufs["obs"])
        for k, v in got.items():
            assert bufs[k].download(v.dtype, v.size).tobytes() == v.tobytes() == again[k].tobytes(), k
        for buf in list(bufs.values()) + [d_sc, d_w]:
            buf.free()
    finally:
        d_pl.free()


def test_estimate_without_a_decision(rx):
    """align_bits = 0: the observations and the estimate alone"""
    dev_args, host_args, kw = make_case(2, 3, 3, 16, 4, 8, 3.0, 1.0, 0.5, 0, "hadamard")
    want, got = er.irs_estimate(*host_args, **kw), rx.irs_estimate(*dev_args, **kw)
    assert sorted(got) == ["est", "obs"]
    compare(got, want, 0)


def test_every_subset_of_the_outputs(rx):
    M, L, n_sets, N, G, T, guard = 2, 9, 3, 16, 4, 17, 64                  # 54 rows: tiles that straddle the sets
    dev_args, host_args, kw = make_case(M, L, n_sets, N, G, T, 3.0, 1.0, 0.5, 2, "any")
    want = er.irs_estimate(*host_args, **kw)
    names = ("taps", "est", "codes", "obs")
    ptr_kw = {"taps": None, "est": "est_ptr", "codes": "codes_ptr", "obs": "obs_ptr"}
    d_sc = rx.alloc(kw["scatter"].nbytes).upload(kw["scatter"])
    d_w = rx.alloc(kw["noise"].nbytes).upload(kw["noise"])
    call_kw = dict(kw, scatter=d_sc, n_scatter=kw["scatter"].shape[0], noise=d_w, n_noise=kw["noise"].shape[0])
    try:
        for mask in range(1, 16):
            asked = [n for i, n in enumerate(names) if mask >> i & 1]
            bufs = {n: rx.alloc(want[n].nbytes + guard).upload(np.full(want[n].nbytes + guard, 0xA5, np.uint8)) for n in names}
            rx.irs_estimate_dev(bufs["taps"] if "taps" in asked else None, *dev_args,
                                **{ptr_kw[n]: bufs[n] for n in asked if ptr_kw[n]}, **call_kw)
            for n in names:
                raw = bufs[n].download(np.uint8, want[n].nbytes + guard)
                bufs[n].free()
                assert (raw[want[n].nbytes:] == 0xA5).all(), (asked, n, "the guard region")
                if n in asked:
                    assert raw[:want[n].nbytes].tobytes() == want[n].tobytes(), (asked, n)
                else:
                    assert (raw[:want[n].nbytes] == 0xA5).all(), (asked, n, "written without being asked for")
    finally:
        d_sc.free()
        d_w.free()


# ---- 2. kernel against kernel ----

@pytest.mark.parametrize("M,L,n_sets,N,G,T", [(1, 3, 7, 65, 65, 17), (3, 6, 3, 16, 4, 5), (8, 16, 2, 65, 14, 65)])
def test_against_the_sweep_and_the_cascade(rx, M, L, n_sets, N, G, T):
    rng = np.random.default_rng(7 * M + N + T)
    a, b, d, pdp, sc = scene(rng, M, N, L, n_sets * L)
    pl = any_pilots(rng, T, G)
    gm = None if G == N else (irs.groups(4, 2) if (N, G) == (16, 4) else any_groups(rng, N, G))
    kw = dict(gain=0.7, k_factor=3.0)
    for src in (dict(scatter=sc), dict(seed=0x1234567890)):
        got = rx.irs_estimate(n_sets, pdp, a, b, d, pilots=pl, group=gm, sigma=0.0, align_bits=2, **kw, **src)
        # the observation of slot t is rule 28's tap of the codebook entry t = the group-expanded pilot row
        sw = rx.irs_sweep_multi(n_sets, pdp, a, b, d, codebook=er.expand(pl, er.group_map(gm, N, G)), **kw, **src)
        o = got["obs"]
        q = o.real * o.real + o.imag * o.imag                                     # two products and one add, each rounded
        assert same(mr.power_sum(q), sw["power"])
        # the taps are rule 27's under the phases of the decided codes
        psi = irs.PHASES[got["codes"][:, er.group_map(gm, N, G)].astype(np.intp) << 1]
        casc = rx.irs_taps_multi(n_sets, pdp, a, b, d, psi=psi, **kw, **src)
        assert got["taps"].tobytes() == casc.tobytes()
    one = rx.irs_estimate(n_sets, pdp, a[0], b, d[:1], pilots=pl, group=gm, sigma=0.0, align_bits=3, seed=5, **kw)
    psi = irs.PHASES[one["codes"][:, er.group_map(gm, N, G)].astype(np.intp)]
    assert one["taps"][0].tobytes() == rx.irs_taps(n_sets, pdp, a[0], b, d[0], psi=psi, seed=5, **kw).tobytes()


# ---- 3. Philox scatter and noise ----

@pytest.mark.parametrize("M,N,L,n_sets,T", [(4, 65, 3, 5, 17), (1, 16, 1, 7, 5)])
def test_philox_scatter_and_noise(rx, M, N, L, n_sets, T):
    rng = np.random.default_rng(N + M)
    a, b, d, pdp, _ = scene(rng, M, N, L, 1)
    pl = any_pilots(rng, T, N)
    w = crandn(rng, n_sets * M * L, T)
    seed = 0xFEDCBA9876543210
    for k_factor in (0.0, 10.0):
        # the direct path is blocked (it would be one more draw through the device's own Box-Muller); the device's elements go
        # into the restatement, and the rest of the rule is exact
        kw = dict(k_factor=k_factor, direct_gain=0.0, seed=seed)
        el = rx.irs_taps_multi(n_sets, pdp, a, b, None, psi=np.ones(N, np.complex64), want_elems=True, **kw)["elems"]
        est = dict(pilots=pl, sigma=0.5, align_bits=2, noise=w)
        got = rx.irs_estimate(n_sets, pdp, a, b, None, **est, **kw)
        compare(got, er.irs_estimate(n_sets, pdp, a, b, None, elems=el, **est, **kw), 2)
        # the drawn noise: the counters (t, r, rho, 3) through the device's logf / sincosf, within rule 25's 1e-5 per unit sigma
        for sigma in (1.0, 3.0):
            drawn = rx.irs_estimate(n_sets, pdp, a, b, None, pilots=pl, sigma=sigma, want=("obs",), **kw)["obs"]
            host = er.irs_estimate(n_sets, pdp, a, b, None, pilots=pl, sigma=sigma, elems=el, **kw)["obs"]
            lim = 1e-5 * sigma + 2.0 ** -23 * np.abs(host)
            assert (np.abs(drawn.real - host.real) <= lim).all() and (np.abs(drawn.imag - host.imag) <= lim).all()
            assert drawn.tobytes() == rx.irs_estimate(n_sets, pdp, a, b, None, pilots=pl, sigma=sigma, want=("obs",), **kw)["obs"].tobytes()
        noise = (drawn - got["obs"] + np.float32(0.5) * w.reshape(got["obs"].shape)) / np.float32(3.0)
        assert abs(float((np.abs(noise) ** 2).mean()) - 1.0) < 5.0 / math.sqrt(noise.size)
        other = rx.irs_estimate(n_sets, pdp, a, b, None, pilots=pl, sigma=3.0, want=("obs",), **dict(kw, seed=seed + 1))["obs"]
        assert np.unique(other - drawn).size > other.size // 2


# ---- 4. chained on the device ----

def test_estimate_feeds_the_channel_without_a_sync(rx):
    M, n_rows, row_len, S, L = 2, 5, 200, 4, 3
    rng = np.random.default_rng(6)
    x = cnoise(rng, n_rows * row_len).reshape(n_rows, row_len)
    b2r, r2u, b2u = irs.los(S, [0.015, 0.015, 0], [0.06, 0.06, 4.5], [0.36, -0.14, 1.0], antennas=M)
    pdp = np.exp(-np.arange(L) / 2.0)
    pl = irs.hadamard_pilots(4)
    est = dict(pilots=pl, group=irs.groups(S, 2), sigma=0.5, align_bits=2, gain=1.0 / S, k_factor=1.0, seed=3)
    d_taps, d_in = rx.alloc(M * n_rows * L * 8), rx.alloc(x.nbytes).upload(x)
    d_out = [rx.alloc(x.nbytes) for _ in range(M)]
    try:
        runs = []
        for synced in (False, True):
            d_taps.upload(np.zeros(M * n_rows * L, np.complex64))
            rx.irs_estimate_dev(d_taps, n_rows, pdp / pdp.sum(), b2r, r2u, b2u, **est)
            for m in range(M):
                if synced:
                    rx.sync()
                rx.channel_dev(d_in.ptr, d_out[m].ptr, x.size, n_rows, row_len=row_len, taps=d_taps.ptr + m * n_rows * L * 8,
                               n_taps=L, n_tap_sets=n_rows, cfo=np.float32(0.01))
            runs.append([d_out[m].download(np.complex64, x.size).reshape(n_rows, row_len) for m in range(M)])
        taps = d_taps.download(np.complex64, M * n_rows * L).reshape(M, n_rows, L)
        assert np.isfinite(taps).all() and len(np.unique(taps)) == taps.size
        for m in range(M):
            assert runs[0][m].tobytes() == runs[1][m].tobytes(), m
            assert same(runs[0][m], channel_ref.channel(x, taps=taps[m], cfo=np.float32(0.01))), m
    finally:
        for buf in [d_taps, d_in] + d_out:
            buf.free()


def test_block_trains_per_draw(rx):
    """channel_model(irs=IrsConfig(pilots=...)): every tap set is trained from its own noisy estimate; irs_codes holds the codes"""
    cfg = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0), k_factor=0.5,
               pdp=(0.6, 0.3, 0.1), seed=11, refresh=700, antennas=2, pilots=irs.hadamard_pilots(4), group=irs.groups(4, 2),
               pilot_sigma=0.5, pilot_bits=2)
    c = irs.IrsConfig(**cfg)
    direct = rx.irs_estimate(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, pilots=c.pilots, group=c.group, sigma=0.5, align_bits=2,
                             k_factor=0.5, seed=11, want=("taps", "codes"))
    n = 1500
    x = cnoise(np.random.default_rng(12), n)
    blk = block.channel_model(noise_voltage=0.0, irs=c)
    try:
        assert len(blk.out_sig) == 2 and blk.irs_codes.shape == (0, 4)
        got = np.zeros((2, n), np.complex64)
        assert blk.work([x[:900]], [got[0, :900], got[1, :900]]) == 900
        assert blk.work([x[900:]], [got[0, 900:], got[1, 900:]]) == n - 900
        assert np.array_equal(blk.irs_codes[:16], direct["codes"])
        with pytest.raises(ValueError):
            blk.set_psi(np.ones(16))
        with pytest.raises(ValueError):
            blk.irs_best
    finally:
        blk.close()
    for m in range(2):       # sample t runs through set t // refresh of plane m
        sets = direct["taps"][m, np.arange(n) // 700]
        coef = [(sets[:, l].real.copy(), sets[:, l].imag.copy()) for l in range(3)]
        assert same(got[m], channel_ref.mix(*channel_ref.fir(x, coef), inc=0, noise_voltage=0.0)), m


# ---- 5. end to end ----

def device_point(rx, sigma):
    import irs_estimate_point as pt
    (pdp, a, b), kw = pt.scene()
    pl, kappa = pt.pilots()
    est = rx.irs_estimate(pt.N_SETS, pdp, a, b, None, pilots=pl, sigma=sigma, est_scale=kappa, align_bits=pt.BITS,
                          want=("taps", "codes"), **kw)
    genie = rx.irs_taps_multi(pt.N_SETS, pdp, a, b, None, align_bits=pt.BITS, want_codes=True, **kw)
    rand = rx.irs_taps_multi(pt.N_SETS, pdp, a, b, None, psi=irs.random_psi(pt.N_ELEMS, pt.BITS, pt.PSI_SEED), **kw)
    return est, genie, pt.power(est["taps"]), pt.power(genie["taps"]), pt.power(rand)


def test_trained_surface_between_random_and_genie(rx):
    """N = 64, B = 2, k_factor = 0, the direct path blocked, 256 sets, 65 DFT pilots.  Without noise the trained surface collects the
    genie's mean power: a code differs from the genie's only where an element lies within the estimate's float32 error of a
    decision boundary, where both codes add the same power to that error, so 1e-6 of the power is allowed (and the codes are
    held to the cap in test_codes_at_sigma_zero_direct_blocked).  At the sigma that tests/irs_estimate_point.py chose the ratio to
    the genie is the recorded one +- 5 of its standard errors, above the random surface's and below the genie's."""
    import irs_estimate_point as pt
    with open(os.path.join(ROOT, "profiles", "irs_estimate_operating_point.json")) as f:
        rec = json.load(f)
    assert rec["chosen_sigma"] == pt.SIGMA and abs(rec["chosen"]["ratio"] - rec["target"]) < 0.05
    _, _, p_est, p_gen, p_rnd = device_point(rx, 0.0)
    r0, se0 = pt.ratio(p_est, p_gen)
    print("sigma = 0: power / genie's = %.4f +- %.4f (host %.4f)" % (r0, se0, rec["points"][0]["ratio"]))
    assert abs(r0 - 1.0) <= 1e-6
    _, _, p_est, p_gen, p_rnd = device_point(rx, pt.SIGMA)
    r, se = pt.ratio(p_est, p_gen)
    print("sigma = %g: power / genie's = %.4f +- %.4f (host %.4f +- %.4f), random %.4f"
          % (pt.SIGMA, r, se, rec["chosen"]["ratio"], rec["chosen"]["ratio_se"], pt.ratio(p_rnd, p_gen)[0]))
    assert p_rnd.mean() < p_est.mean() < p_gen.mean()
    assert abs(r - rec["chosen"]["ratio"]) <= 5 * rec["chosen"]["ratio_se"]


def test_codes_at_sigma_zero_with_a_direct_path(rx):
    """the same surface with the direct path present (direct_gain = 1): at sigma = 0 the codes decided from the estimate are the
    genie's except in at most 1 element in 1000, and where none differs the taps are the genie's bytes"""
    import irs_estimate_point as pt
    (pdp, a, b), kw = pt.scene()
    kw = dict(kw, direct_gain=1.0)
    d = np.ones(1, np.complex64)
    pl, kappa = pt.pilots()
    est = rx.irs_estimate(pt.N_SETS, pdp, a, b, d, pilots=pl, sigma=0.0, est_scale=kappa, align_bits=pt.BITS, want=("taps", "codes"), **kw)
    genie = rx.irs_taps_multi(pt.N_SETS, pdp, a, b, d, align_bits=pt.BITS, want_codes=True, **kw)
    differ = int((est["codes"] != genie["codes"]).sum())
    print("%d of %d codes differ from the genie's" % (differ, genie["codes"].size))
    assert differ * 1000 <= genie["codes"].size
    clean = (est["codes"] == genie["codes"]).all(axis=1)
    assert est["taps"][:, clean].tobytes() == genie["taps"][:, clean].tobytes()


def test_codes_at_sigma_zero_direct_blocked(rx):
    """The issue's condition: N = 64, B = 2, k_factor = 0, the direct path blocked, 256 sets, sigma = 0: the codes equal the
    genie's except in at most 1 element in 1000.  With direct_gain = 0 rule 29 does not consult the estimate of the direct path
    (which is then nothing but noise and rounding) and aligns to the positive real axis, as rule 25's genie does; the sets
    without a differing code have the genie's taps byte for byte."""
    est, genie, p_est, p_gen, _ = device_point(rx, 0.0)
    differ = int((est["codes"] != genie["codes"]).sum())
    print("%d of %d codes differ from the genie's" % (differ, genie["codes"].size))
    assert differ * 1000 <= genie["codes"].size
    clean = (est["codes"] == genie["codes"]).all(axis=1)
    assert est["taps"][:, clean].tobytes() == genie["taps"][:, clean].tobytes()
