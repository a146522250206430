"""wifirx_irs_optimize_weighted, the joint phase decision with a signed weight on every row (wr_irs_optimize.hip, NUMERICS.md rule
31), on the device:
  * host-built coefficient matrices and weights: codes, phases, power trace and sweep count bit for bit tests/irs_optimize_w_ref.py,
    over R 1 / 3 / 64 / 65 / 128 (the lane pairing of the weights), G on both sides of the 8-column chunk and of two chunks,
    1 / 5 / 130 sets (four sets share a workgroup), B = 1, 2, 3, 0 / 1 / 4 / 16 sweeps, the three starts, blocked and not, and
    every kind of weight: random signed, (1, 0, ..) tiled over the antennas, one negative row, all zero; host [R], device [1][R],
    device [n_sets][R] with other rows per set;
  * the properties that hold exactly, on the device: w = 1 against wifirx_irs_optimize output for output, w = 4, rows of weight
    zero that hold NaN and infinities against the same rows zeroed and against fewer rows; a NaN device weight;
  * every subset of the outputs, sentinels;
  * estimate -> weighted optimize -> taps_multi queued without a sync, against the same with syncs and against the restatements;
  * channel_model(irs=IrsConfig(decision="joint", tap_weights=(1, 0)))."""
import math

import numpy as np
import pytest

import irs_estimate_ref as er
import irs_multi_ref as mr
import irs_optimize_w_ref as wrf
from channel_helpers import cnoise, rx, same  # noqa: F401 (rx: fixture)
from wifirx import block, irs

pytestmark = pytest.mark.gpu

START = {wrf.START_REF: "ref", wrf.START_GIVEN: "given", wrf.START_ZERO: "zero"}
NAMES = ("codes", "psi", "power", "sweeps")


def crandn(rng, *shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * math.sqrt(0.5)).astype(np.complex64)


def compare(got, want, bits):
    assert np.array_equal(got["codes"], want["codes"]) and (got["codes"] < (1 << bits)).all(), "codes"
    assert same(got["psi"], want["psi"]), "psi"
    nan = np.isnan(want["power"])                                      # a NaN is a NaN: its sign and payload are not the rule's
    assert np.array_equal(np.isnan(got["power"]), nan) and same(np.where(nan, 0, got["power"]), np.where(nan, 0, want["power"])), "power"
    assert np.array_equal(got["sweeps"], want["sweeps"]), "sweeps"


def identical(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def weights(kind, rng, R, n_sets):
    """float32 [R], or [n_sets, R] for the per-set kinds"""
    if kind == "signed":
        return rng.standard_normal(R).astype(np.float32)
    if kind == "tap0":                                                 # (1, 0, ..) per antenna: L = 4 where it divides R
        L = 4 if R % 4 == 0 else R
        return irs.row_weights(R // L, L, tap=irs.tap_weights(L))
    if kind == "one_negative":
        w = np.ones(R, np.float32)
        w[R - 1] = -0.75
        return w
    if kind == "zero":
        return np.zeros(R, np.float32)
    if kind == "per_set":                                              # other rows per set, zeros and both signs among them
        w = rng.standard_normal((n_sets, R)).astype(np.float32)
        w[rng.random((n_sets, R)) < 0.2] = 0
        return w
    raise ValueError(kind)


def run(rx, q, w, bits, sweeps, start=wrf.START_REF, blocked=False, ci=None, group=None, device=False):
    """the device call; device=True sends a [R] weight vector as a device buffer of one row block"""
    kw = dict(bits=bits, max_sweeps=sweeps, start=START[start], direct_blocked=blocked,
              codes_in=ci if start == wrf.START_GIVEN else None, group=group)
    if not device:
        return rx.irs_optimize(q, weights=w, **kw)
    w = np.ascontiguousarray(w, dtype=np.float32)
    n_sets, R, J = q.shape
    N = J - 1 if group is None else np.asarray(group).size
    shapes = {"codes": (np.uint8, (n_sets, J - 1)), "psi": (np.complex64, (n_sets, N)), "power": (np.float32, (n_sets, sweeps + 1)),
              "sweeps": (np.uint8, (n_sets,))}
    bufs = {"q": rx.alloc(q.nbytes).upload(q), "w": rx.alloc(w.nbytes).upload(w)}
    try:
        for n, (dt, sh) in shapes.items():
            bufs[n] = rx.alloc(max(int(np.prod(sh)) * np.dtype(dt).itemsize, 8))
        if kw["codes_in"] is not None:
            bufs["ci"] = rx.alloc(ci.nbytes).upload(np.ascontiguousarray(ci))
        kw["codes_in"] = bufs.get("ci")
        rx.irs_optimize_dev(bufs["q"], n_sets, R, J, n_elems=N, weights_ptr=bufs["w"], n_weight_sets=1,
                            **{n + "_ptr": bufs[n] for n in NAMES}, **kw)
        return {n: bufs[n].download(dt, int(np.prod(sh))).reshape(sh) for n, (dt, sh) in shapes.items()}
    finally:
        for b in bufs.values():
            b.free()


# ---- 1. kernel against restatement ----

#          R    G   sets bits sweeps start            blocked  weights        device [1][R]
CASES = [(1, 1, 1, 1, 0, wrf.START_REF, False, "signed", False), (1, 1, 5, 2, 4, wrf.START_ZERO, True, "one_negative", True),
         (1, 1, 130, 3, 1, wrf.START_GIVEN, False, "per_set", False), (3, 7, 130, 2, 4, wrf.START_REF, False, "signed", True),
         (3, 7, 5, 3, 1, wrf.START_GIVEN, True, "per_set", False), (3, 7, 1, 1, 16, wrf.START_ZERO, False, "one_negative", False),
         (64, 8, 5, 3, 4, wrf.START_REF, True, "tap0", False), (64, 8, 1, 1, 1, wrf.START_ZERO, False, "signed", True),
         (64, 8, 5, 2, 0, wrf.START_GIVEN, True, "per_set", False), (65, 9, 5, 2, 4, wrf.START_GIVEN, False, "signed", False),
         (65, 9, 1, 3, 0, wrf.START_ZERO, True, "one_negative", True), (65, 9, 5, 1, 16, wrf.START_REF, False, "per_set", False),
         (128, 17, 130, 2, 1, wrf.START_ZERO, True, "signed", False), (128, 17, 5, 1, 4, wrf.START_REF, True, "tap0", True),
         (128, 17, 1, 3, 4, wrf.START_GIVEN, False, "per_set", False), (128, 9, 5, 2, 4, wrf.START_REF, False, "one_negative", False),
         (8, 7, 5, 2, 4, wrf.START_REF, False, "tap0", False), (65, 8, 5, 2, 4, wrf.START_GIVEN, False, "zero", False),
         (3, 1, 5, 3, 4, wrf.START_REF, True, "zero", True), (100, 23, 6, 2, 4, wrf.START_REF, False, "per_set", False)]


@pytest.mark.parametrize("R,G,n_sets,bits,sweeps,start,blocked,kind,device", CASES)
def test_kernel_equals_the_restatement(rx, R, G, n_sets, bits, sweeps, start, blocked, kind, device):
    rng = np.random.default_rng(31000 + 1000 * R + 10 * G + n_sets + bits)
    q = crandn(rng, n_sets, R, G + 1)
    ci = rng.integers(0, 256, (n_sets, G)).astype(np.uint8)            # only the low B bits count
    w = weights(kind, rng, R, n_sets)
    want = wrf.optimize(q, bits, sweeps, start, blocked, ci, weights=w)
    got = run(rx, q, w, bits, sweeps, start, blocked, ci, device=device)
    assert got["power"].shape == (n_sets, sweeps + 1) and got["psi"].shape == (n_sets, G)
    compare(got, want, bits)
    if kind == "zero" and sweeps:                                      # z = +0 at every step: every code becomes 0 in sweep 1
        assert not got["codes"].any() and got["power"].tobytes() == bytes(got["power"].nbytes)
        assert (got["sweeps"] <= 1).all()


def test_weighted_decision_differs_from_the_unweighted_one(rx):
    """the cases above would pass on a kernel that ignored its weights only if the weights never mattered: here they do"""
    rng = np.random.default_rng(3101)
    q = crandn(rng, 5, 65, 10)
    w = weights("signed", rng, 65, 5)
    got = rx.irs_optimize(q, bits=2, max_sweeps=4, weights=w)
    plain = rx.irs_optimize(q, bits=2, max_sweeps=4)
    assert (got["codes"] != plain["codes"]).any() and (got["power"] != plain["power"]).any()
    flipped = w.copy()
    flipped[64] = -flipped[64]                                         # the one row of the upper half: its weight is read
    assert not identical(got, rx.irs_optimize(q, bits=2, max_sweeps=4, weights=flipped))
    compare(got, wrf.optimize(q, 2, 4, weights=w), 2)


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_groups(rx, bits):
    """psi_out through the map of groups(4, 2), the group map and the host weights in one upload"""
    rng = np.random.default_rng(3140 + bits)
    q, w = crandn(rng, 5, 3, 5), weights("signed", rng, 3, 5)
    got = run(rx, q, w, bits, 4, group=irs.groups(4, 2))
    assert got["psi"].shape == (5, 16)
    compare(got, wrf.optimize(q, bits, 4, group=irs.groups(4, 2), weights=w), bits)


# ---- 2. the properties that hold exactly ----

def test_unit_weights_are_the_unweighted_call(rx):
    rng = np.random.default_rng(3102)
    for R, G, bits, n_sets in ((5, 9, 2, 6), (64, 8, 3, 4), (65, 17, 1, 5), (128, 7, 2, 3)):
        q = crandn(rng, n_sets, R, G + 1)
        if R == 65:
            q[1, 64, 3] = np.nan                                       # a NaN stays a NaN
        base = rx.irs_optimize(q, bits=bits, max_sweeps=4)
        one = np.ones(R, np.float32)
        for got in (rx.irs_optimize(q, bits=bits, max_sweeps=4, weights=one), run(rx, q, one, bits, 4, device=True),
                    rx.irs_optimize(q, bits=bits, max_sweeps=4, weights=np.ones((n_sets, R), np.float32))):
            assert np.array_equal(np.isnan(got["power"]), np.isnan(base["power"]))
            assert all(np.nan_to_num(got[k]).tobytes() == np.nan_to_num(base[k]).tobytes() for k in NAMES), (R, G)
        four = rx.irs_optimize(q, bits=bits, max_sweeps=4, weights=np.full(R, 4, np.float32))
        assert np.array_equal(four["codes"], base["codes"]) and np.array_equal(four["sweeps"], base["sweeps"])
        assert same(np.nan_to_num(four["power"]), np.nan_to_num(4 * base["power"]))


def test_rows_of_weight_zero_are_absent(rx):
    """rows of weight zero (either sign) that hold NaN and infinities, on both sides of row 64: the bits of the same call with
    those rows zeroed, and, where they are the last rows, of the call with fewer rows"""
    rng = np.random.default_rng(3103)
    for R, dead, bits, start in ((70, (3, 40, 66, 69), 2, wrf.START_ZERO), (128, (1, 63, 64, 127), 3, wrf.START_REF),
                                 (9, (5,), 1, wrf.START_GIVEN)):
        q, w = crandn(rng, 5, R, 12), rng.standard_normal(R).astype(np.float32)
        ci = rng.integers(0, 8, (5, 11)).astype(np.uint8)
        w[list(dead)] = [0.0, -0.0, 0.0, -0.0][:len(dead)]
        bad, zeroed = q.copy(), q.copy()
        bad[:, list(dead)] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e38], np.float32), (5, len(dead), 12))
        zeroed[:, list(dead)] = 0
        a, b = run(rx, bad, w, bits, 4, start, ci=ci), run(rx, zeroed, w, bits, 4, start, ci=ci)
        assert identical(a, b) and np.isfinite(a["power"]).all(), R
        compare(a, wrf.optimize(bad, bits, 4, start, codes_in=ci, weights=w), bits)
    for R, keep in ((70, 64), (70, 66), (128, 5), (64, 63)):           # trailing rows: the call with fewer rows
        q, w = crandn(rng, 5, R, 10), rng.standard_normal(R).astype(np.float32)
        w[keep:] = 0
        q[:, keep:] = np.nan
        a, b = run(rx, q, w, 2, 4), run(rx, np.ascontiguousarray(q[:, :keep]), w[:keep], 2, 4)
        assert identical(a, b), (R, keep)


def test_nan_device_weight(rx):
    """device weights are not inspected: w != 0 holds for a NaN, the row's terms are NaN, and no NaN replaces the maximum"""
    rng = np.random.default_rng(3104)
    q, w = crandn(rng, 3, 66, 9), rng.standard_normal((3, 66)).astype(np.float32)
    w[1, 65], w[2, 2] = np.nan, np.inf
    got = rx.irs_optimize(q, bits=2, max_sweeps=3, weights=w)
    compare(got, wrf.optimize(q, 2, 3, weights=w), 2)
    assert np.isnan(got["power"][1]).all() and np.isfinite(got["power"][0]).all()


def test_every_subset_of_the_outputs_and_sentinels(rx):
    n_sets, R, G, bits, S, guard = 6, 66, 9, 2, 3, 64
    rng = np.random.default_rng(3105)
    q, grp, w = crandn(rng, n_sets, R, G + 1), rng.integers(0, G, 20).astype(np.uint16), weights("per_set", rng, R, n_sets)
    want = wrf.optimize(q, bits, S, group=grp, weights=w)
    d_q, d_w = rx.alloc(q.nbytes).upload(q), rx.alloc(w.nbytes).upload(w)
    try:
        for mask in range(1, 16):
            asked = [n for i, n in enumerate(NAMES) if mask >> i & 1]
            if "codes" not in asked and "psi" not in asked:
                continue
            bufs = {n: rx.alloc(want[n].nbytes + guard).upload(np.full(want[n].nbytes + guard, 0xA5, np.uint8)) for n in NAMES}
            rx.irs_optimize_dev(d_q, n_sets, R, G + 1, bits=bits, max_sweeps=S, group=grp, weights_ptr=d_w, n_weight_sets=n_sets,
                                **{n + "_ptr": bufs[n] for n in asked})
            for n in NAMES:
                raw = bufs[n].download(np.uint8, want[n].nbytes + guard)
                bufs[n].free()
                assert (raw[want[n].nbytes:] == 0xA5).all(), (asked, n, "the guard region")
                if n in asked:
                    assert raw[:want[n].nbytes].tobytes() == want[n].tobytes(), (asked, n)
                else:
                    assert (raw[:want[n].nbytes] == 0xA5).all(), (asked, n, "written without being asked for")
        assert d_q.download(np.complex64, q.size).tobytes() == q.tobytes()      # the coefficients and the weights are read only
        assert d_w.download(np.float32, w.size).tobytes() == w.tobytes()
    finally:
        d_q.free()
        d_w.free()


# ---- 3. the pipeline ----

def estimate_case(rng, M, L, n_sets, N, T, dg, sigma):
    pdp = np.exp(-np.arange(L) / 3.0).astype(np.float32)
    a, b, d = crandn(rng, M, N), crandn(rng, N), crandn(rng, M)
    sc, w = crandn(rng, n_sets * L, (M + 1) * N + M), crandn(rng, n_sets * M * L, T)
    kw = dict(pilots=irs.dft_pilots(N), group=None, sigma=sigma, gain=1.3, k_factor=2.0, direct_gain=dg, scatter=sc, noise=w)
    return (n_sets, pdp, a, b, d if dg else None), (n_sets, pdp, a, b, d), kw


def test_estimate_weighted_optimize_taps_without_a_sync(rx):
    """given scatter and given noise, M = 4, L = 2, N = 16, 64 sets, w = (1, -0.5) per antenna: the three calls queued back to
    back give the bytes of the same calls with a sync between them, and the restatements' taps bit for bit"""
    M, L, n_sets, N, bits, S = 4, 2, 64, 16, 2, 4
    dev_args, host_args, kw = estimate_case(np.random.default_rng(3113), M, L, n_sets, N, N + 1, 1.0, 0.7)
    R, J = M * L, N + 1
    w = irs.row_weights(M, L, tap=irs.tap_weights(L, penalty=0.5))
    assert w.tolist() == [1, -0.5] * M
    ref = er.irs_estimate(*host_args, **kw)
    opt = wrf.optimize(ref["est"], bits, S, weights=w)
    scene = dict(gain=kw["gain"], k_factor=kw["k_factor"], direct_gain=kw["direct_gain"], scatter=kw["scatter"])
    want = mr.irs_taps_multi(*host_args, psi=opt["psi"], **scene)["taps"]
    assert (opt["codes"] != wrf.optimize(ref["est"], bits, S)["codes"]).any()       # the weights decide otherwise
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
            rx.irs_optimize_dev(bufs["est"], n_sets, R, J, bits=bits, max_sweeps=S, codes_ptr=bufs["codes"], psi_ptr=bufs["psi"],
                                weights=w)
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


def test_block_decides_with_tap_weights(rx):
    """channel_model(irs=IrsConfig(decision="joint", tap_weights=(1, 0))): irs_codes are the restatement's on the device's
    estimate, and other codes than the unweighted joint decision's"""
    cfg = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0), k_factor=0.5,
               pdp=(0.6, 0.4), seed=11, refresh=700, antennas=2, pilots=irs.hadamard_pilots(4), group=irs.groups(4, 2),
               pilot_sigma=0.5, pilot_bits=2)
    c = irs.IrsConfig(decision="joint", sweeps=3, tap_weights=(1, 0), **cfg)
    assert c.row_weights.tolist() == [1, 0, 1, 0]
    est = rx.irs_estimate(16, c.pdp, c.los_b2r, c.los_r2u, c.los_b2u, pilots=c.pilots, group=c.group, sigma=0.5, align_bits=2,
                          want=("est",), k_factor=0.5, seed=11)
    want = wrf.optimize(est["est"], 2, 3, group=c.group, weights=c.row_weights)
    plain = wrf.optimize(est["est"], 2, 3, group=c.group)
    assert (want["codes"] != plain["codes"]).any()
    x = cnoise(np.random.default_rng(12), 1500)
    blk = block.channel_model(noise_voltage=0.0, irs=c)
    try:
        got = np.zeros((2, 1500), np.complex64)
        assert blk.work([x], [got[0], got[1]]) == 1500
        assert np.array_equal(blk.irs_codes[:16], want["codes"])
    finally:
        blk.close()
