"""wifirx_irs_optimize, the joint phase decision over antennas and taps (wr_irs_optimize.hip, NUMERICS.md rule 30), on the device:
  * host-built coefficient matrices: codes, phases, power trace and sweep count bit for bit tests/irs_optimize_ref.py, over the
    shapes at which the kernel can go wrong (R 1 / 3 / 64 / 65 / 128, G on both sides of the 8-column chunk and of two chunks,
    the caps R = 128 with G = 1023), B = 1, 2, 3, 0 / 1 / 4 sweeps, the three starts, blocked and not, 1 / 5 / 130 sets (four
    sets share a workgroup), identity groups and groups(4, 2);
  * special inputs (a zero set, exact ties, a NaN row) and the invariants that hold exactly (rows copied into the upper half,
    zero rows, scaling by 4), on the device;
  * equality with wifirx_irs_estimate's decision at max_sweeps = 0, every subset of the outputs, sentinels;
  * estimate -> optimize -> taps_multi queued without a sync, against the same with syncs and against the restatements;
  * channel_model(irs=IrsConfig(decision="joint"))."""
import math

import numpy as np
import pytest

import channel_ref
import irs_estimate_ref as er
import irs_multi_ref as mr
import irs_optimize_ref as orf
from channel_helpers import cnoise, rx, same  # noqa: F401 (rx: fixture)
from wifirx import block, capi, irs

pytestmark = pytest.mark.gpu

START = {orf.START_REF: "ref", orf.START_GIVEN: "given", orf.START_ZERO: "zero"}


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def compare(got, want, bits):
    assert np.array_equal(got["codes"], want["codes"]) and (got["codes"] < (1 << bits)).all(), "codes"
    assert same(got["psi"], want["psi"]), "psi"
    nan = np.isnan(want["power"])                                      # a NaN is a NaN: its sign and payload are not the rule's
    assert np.array_equal(np.isnan(got["power"]), nan) and same(np.where(nan, 0, got["power"]), np.where(nan, 0, want["power"])), "power"
    assert np.array_equal(got["sweeps"], want["sweeps"]), "sweeps"


def both(rx, q, bits, sweeps, start=orf.START_REF, blocked=False, ci=None, group=None):
    want = orf.optimize(q, bits, sweeps, start, blocked, ci, group=group)
    got = rx.irs_optimize(q, bits=bits, max_sweeps=sweeps, start=START[start], direct_blocked=blocked,
                          codes_in=ci if start == orf.START_GIVEN else None, group=group)
    return got, want


# ---- 1. kernel against restatement ----

#          R    G   sets bits sweeps start            blocked
CASES = [(1, 1, 1, 1, 0, orf.START_REF, False), (1, 1, 5, 2, 4, orf.START_ZERO, True), (1, 1, 130, 3, 1, orf.START_GIVEN, False),
         (3, 4, 130, 2, 4, orf.START_REF, False), (3, 4, 5, 3, 1, orf.START_GIVEN, True), (3, 4, 1, 1, 4, orf.START_ZERO, False),
         (64, 7, 5, 3, 4, orf.START_REF, True), (64, 7, 1, 1, 1, orf.START_ZERO, False), (64, 7, 5, 2, 0, orf.START_GIVEN, True),
         (65, 8, 5, 2, 4, orf.START_GIVEN, False), (65, 8, 1, 3, 0, orf.START_ZERO, True), (65, 8, 5, 1, 1, orf.START_REF, False),
         (128, 9, 130, 2, 1, orf.START_ZERO, True), (128, 9, 5, 1, 4, orf.START_REF, True), (128, 9, 1, 3, 4, orf.START_GIVEN, False),
         (17, 64, 5, 2, 4, orf.START_REF, False), (17, 64, 1, 1, 4, orf.START_GIVEN, True), (17, 64, 5, 3, 1, orf.START_ZERO, False),
         (2, 15, 5, 2, 4, orf.START_REF, True), (2, 16, 5, 3, 4, orf.START_ZERO, False), (2, 17, 5, 1, 4, orf.START_GIVEN, False),
         (100, 23, 6, 2, 4, orf.START_REF, False)]


@pytest.mark.parametrize("R,G,n_sets,bits,sweeps,start,blocked", CASES)
def test_kernel_equals_the_restatement(rx, R, G, n_sets, bits, sweeps, start, blocked):
    rng = np.random.default_rng(1000 * R + 10 * G + n_sets + bits)
    q = crandn(rng, n_sets, R, G + 1)
    ci = rng.integers(0, 256, (n_sets, G)).astype(np.uint8)            # only the low B bits count
    got, want = both(rx, q, bits, sweeps, start, blocked, ci)
    assert got["power"].shape == (n_sets, sweeps + 1) and got["psi"].shape == (n_sets, G)
    compare(got, want, bits)


def test_the_caps(rx):
    """R = 128, G = 1023 (J = 1024), two sets, 16 sweeps allowed"""
    q = crandn(np.random.default_rng(7), 2, 128, 1024)
    got, want = both(rx, q, 2, 2, orf.START_REF, False)
    compare(got, want, 2)
    q = crandn(np.random.default_rng(8), 3, 4, 6)
    got, want = both(rx, q, 3, 16, orf.START_ZERO, True)
    compare(got, want, 3)
    assert (want["sweeps"] < 16).all()                                 # the early exit was taken


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_groups(rx, bits):
    """psi_out through the map of groups(4, 2): 16 elements behind 4 groups"""
    q = crandn(np.random.default_rng(40 + bits), 5, 3, 5)
    got, want = both(rx, q, bits, 4, group=irs.groups(4, 2))
    assert got["psi"].shape == (5, 16)
    compare(got, want, bits)


# ---- 2. special inputs and invariants ----

def test_special_inputs(rx):
    got, want = both(rx, np.zeros((2, 5, 9), np.complex64), 2, 4)
    compare(got, want, 2)
    assert not got["codes"].any() and got["power"].tobytes() == bytes(got["power"].nbytes) and not got["sweeps"].any()
    # exact ties: z = 1 + j between the codes 0 and 3 of 4; z = 0 among all; the lowest c wins
    tie = np.array([[[1 - 1j, 1]], [[0, 1]]], np.complex64)
    got, want = both(rx, tie, 2, 2, orf.START_ZERO)
    compare(got, want, 2)
    assert not got["codes"].any()
    got, want = both(rx, tie, 2, 2, orf.START_GIVEN, ci=np.array([[3], [3]], np.uint8))
    compare(got, want, 2)
    assert got["codes"].tolist() == [[0], [0]]
    q = crandn(np.random.default_rng(9), 3, 70, 12)
    q[1, 66, 5] = np.nan                                               # a NaN in the upper half of one set; the others are clean
    q[2, 0, 0] = np.inf
    got, want = both(rx, q, 3, 3)
    compare(got, want, 3)
    assert np.isnan(got["power"][1]).all() and np.isfinite(got["power"][0]).all()


def test_invariants_on_the_device(rx):
    rng = np.random.default_rng(10)
    for R, G, bits in ((5, 9, 2), (64, 8, 3), (33, 17, 1)):
        q = crandn(rng, 4, R, G + 1)
        base = rx.irs_optimize(q, bits=bits, max_sweeps=4)
        two = np.zeros((4, 64 + R, G + 1), np.complex64)
        two[:, :R], two[:, 64:] = q, q
        dup = rx.irs_optimize(two, bits=bits, max_sweeps=4)
        assert np.array_equal(dup["codes"], base["codes"]) and same(dup["power"], 2 * base["power"])
        wide = np.concatenate([q, np.zeros((4, 128 - R, G + 1), np.complex64)], axis=1)
        zero = rx.irs_optimize(wide, bits=bits, max_sweeps=4)
        assert all(zero[k].tobytes() == base[k].tobytes() for k in base)
        four = rx.irs_optimize(4 * q, bits=bits, max_sweeps=4)
        assert np.array_equal(four["codes"], base["codes"]) and same(four["power"], 16 * base["power"])


# ---- 3. equality with the existing calls ----

def estimate_case(rng, M, L, n_sets, N, G, T, dg, sigma):
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    a, b, d = crandn(rng, M, N), crandn(rng, N), crandn(rng, M)
    sc, w = crandn(rng, n_sets * L, (M + 1) * N + M), crandn(rng, n_sets * M * L, T)
    gm = None if G == N else irs.groups(4, 2)
    kw = dict(pilots=irs.dft_pilots(G) if T == G + 1 else irs.hadamard_pilots(G), group=gm, sigma=sigma, gain=1.3, k_factor=2.0,
              direct_gain=dg, scatter=sc, noise=w)
    return (n_sets, pdp, a, b, d if dg else None), (n_sets, pdp, a, b, d), kw


@pytest.mark.parametrize("dg", [1.0, 0.0])
def test_no_sweep_is_the_estimate_s_decision(rx, dg):
    dev_args, _, kw = estimate_case(np.random.default_rng(11), 3, 2, 9, 16, 16, 17, dg, 0.5)
    for bits in (1, 2, 3):
        est = rx.irs_estimate(*dev_args, align_bits=bits, want=("est", "codes"), **kw)
        got = rx.irs_optimize(est["est"], bits=bits, max_sweeps=0, start="ref", direct_blocked=dg == 0.0)
        assert np.array_equal(got["codes"], est["codes"])
        assert got["power"].shape == (9, 1) and not got["sweeps"].any()


def test_every_subset_of_the_outputs_and_sentinels(rx):
    n_sets, R, G, bits, S, guard = 6, 66, 9, 2, 3, 64
    rng = np.random.default_rng(12)
    q, grp = crandn(rng, n_sets, R, G + 1), rng.integers(0, G, 20).astype(np.uint16)
    want = orf.optimize(q, bits, S, group=grp)
    names = ("codes", "psi", "power", "sweeps")
    d_q = rx.alloc(q.nbytes).upload(q)
    try:
        for mask in range(1, 16):
            asked = [n for i, n in enumerate(names) if mask >> i & 1]
            if "codes" not in asked and "psi" not in asked:
                continue
            bufs = {n: rx.alloc(want[n].nbytes + guard).upload(np.full(want[n].nbytes + guard, 0xA5, np.uint8)) for n in names}
            rx.irs_optimize_dev(d_q, n_sets, R, G + 1, bits=bits, max_sweeps=S, group=grp, **{n + "_ptr": bufs[n] for n in asked})
            for n in names:
                raw = bufs[n].download(np.uint8, want[n].nbytes + guard)
                bufs[n].free()
                assert (raw[want[n].nbytes:] == 0xA5).all(), (asked, n, "the guard region")
                if n in asked:
                    assert raw[:want[n].nbytes].tobytes() == want[n].tobytes(), (asked, n)
                else:
                    assert (raw[:want[n].nbytes] == 0xA5).all(), (asked, n, "written without being asked for")
        assert d_q.download(np.complex64, q.size).tobytes() == q.tobytes()      # the coefficients are read only
    finally:
        d_q.free()


# ---- 4. the pipeline ----

def test_estimate_optimize_taps_without_a_sync(rx):
    """given scatter and given noise, M = 4, L = 2, N = 16, 64 sets: the three calls queued back to back give the bytes of the
    same calls with a sync between them, and the restatements' taps bit for bit"""
    M, L, n_sets, N, bits, S = 4, 2, 64, 16, 2, 4
    dev_args, host_args, kw = estimate_case(np.random.default_rng(13), M, L, n_sets, N, N, N + 1, 1.0, 0.7)
    R, J = M * L, N + 1
    ref = er.irs_estimate(*host_args, **kw)
    opt = orf.optimize(ref["est"], bits, S)
    scene = dict(gain=kw["gain"], k_factor=kw["k_factor"], direct_gain=kw["direct_gain"], scatter=kw["scatter"])
    want = mr.irs_taps_multi(*host_args, psi=opt["psi"], **scene)["taps"]
    assert (opt["codes"] != er.decide(ref["est"], bits)).any()                 # the joint decision is another one
    d_sc = rx.alloc(kw["scatter"].nbytes).upload(kw["scatter"])
    d_w = rx.alloc(kw["noise"].nbytes).upload(kw["noise"])
    dkw = dict(kw, scatter=d_sc, n_scatter=kw["scatter"].shape[0], noise=d_w, n_noise=kw["noise"].shape[0])
    dscene = dict(scene, scatter=d_sc, n_scatter=kw["scatter"].shape[0])
    bufs = {"est": rx.alloc(n_sets * R * J * 8), "psi": rx.alloc(n_sets * N * 8), "codes": rx.alloc(n_sets * N),
            "taps": rx.alloc(M * n_sets * L * 8)}
    try:
        runs = []
        for sync in (False, True):
            for b in bufs.values():
                b.upload(np.full(b.nbytes, 0xA5, np.uint8))            # nothing of the run before is left
            rx.irs_estimate_dev(None, *dev_args, est_ptr=bufs["est"], **dkw)
            if sync:
                rx.sync()
            rx.irs_optimize_dev(bufs["est"], n_sets, R, J, bits=bits, max_sweeps=S, codes_ptr=bufs["codes"], psi_ptr=bufs["psi"])
            if sync:
                rx.sync()
            rx.irs_taps_multi_dev(bufs["taps"], *dev_args, psi=bufs["psi"], n_psi_sets=n_sets, **dscene)
            runs.append((bufs["taps"].download(np.complex64, M * n_sets * L).reshape(M, n_sets, L),
                         bufs["codes"].download(np.uint8, n_sets * N).reshape(n_sets, N)))
        assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
        assert np.array_equal(runs[0][1], opt["codes"])
        assert same(runs[0][0], want)
    finally:
        for b in list(bufs.values()) + [d_sc, d_w]:
            b.free()


def test_block_decides_jointly(rx):
    """channel_model(irs=IrsConfig(pilots=..., decision="joint")): the taps are those of estimate -> optimize -> taps_multi, and
    irs_codes shows the joint codes; decision="ref" stays what it was"""
    cfg = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0), k_factor=0.5,
               pdp=(0.6, 0.3, 0.1), seed=11, refresh=700, antennas=2, pilots=irs.hadamard_pilots(4), group=irs.groups(4, 2),
               pilot_sigma=0.5, pilot_bits=2)
    c = irs.IrsConfig(decision="joint", sweeps=3, **cfg)
    scene = dict(k_factor=0.5, seed=11)
    est = rx.irs_estimate(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, pilots=c.pilots, group=c.group, sigma=0.5, align_bits=2,
                          want=("est", "codes"), **scene)
    opt = rx.irs_optimize(est["est"], bits=2, max_sweeps=3, group=c.group)
    taps = rx.irs_taps_multi(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, psi=opt["psi"], **scene)
    assert (opt["codes"] != est["codes"]).any()
    n = 1500
    x = cnoise(np.random.default_rng(12), n)
    for cc, codes in ((c, opt["codes"]), (irs.IrsConfig(**cfg), est["codes"])):
        blk = block.channel_model(noise_voltage=0.0, irs=cc)
        try:
            got = np.zeros((2, n), np.complex64)
            assert blk.work([x[:900]], [got[0, :900], got[1, :900]]) == 900
            assert blk.work([x[900:]], [got[0, 900:], got[1, 900:]]) == n - 900
            assert np.array_equal(blk.irs_codes[:16], codes)
        finally:
            blk.close()
        if cc is c:
            for m in range(2):       # sample t runs through set t // refresh of plane m
                sets = taps[m, np.arange(n) // 700]
                coef = [(sets[:, l].real.copy(), sets[:, l].imag.copy()) for l in range(3)]
                assert same(got[m], channel_ref.mix(*channel_ref.fir(x, coef), inc=0, noise_voltage=0.0)), m
