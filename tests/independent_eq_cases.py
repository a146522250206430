"""Cases, tolerances and the comparison shared by tests/test_independent_eq.py (the oracle's SPEC mode on the CPU) and
tests/test_gpu_independent_eq.py (the device): a float32 implementation of the receive chain against the float64
restatement of NUMERICS.md rules 7, 9, 11, 12, 13 in tests/independent_rx.py -- equalised points, LLRs, channel-state
weight, CSI and per-frame moments, for LS / LMS / COMB / STA, at three (bandwidth, frequency) operating points.

Which symbols are compared is decided by the REFERENCE alone.  `m` = the distance of a reference component to the nearest
slicer threshold.  LS, COMB: every point and LLR; decisions where m >= DELTA.  LMS, STA (the decision is fed back): with q
the frame's first symbol that holds a component with m < DELTA (the SIGNAL symbol counts: then nothing of the frame is
compared), symbols <= q are compared, decisions at q only where m >= DELTA; symbols > q are not.  The per-frame moments are
compared on the frames whose symbols are all compared.

The tolerances are 4 x the largest distance measured between the oracle's SPEC mode and the reference over all cases,
equalisers and operating points (profiles/independent_eq_distances.json, written by the CPU test with
WIFIRX_RECORD_DISTANCES=1); the device is held bit-equal to the oracle, so the headroom covers only a change of NumPy /
libm build.  DELTA is 16 x the measured point distance: a decision can flip only inside the rounding distance."""
import os

import numpy as np

from independent_rx import IndependentRx
from wifirx import txgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTANCES = os.path.join(ROOT, "profiles", "independent_eq_distances.json")

TAPS = np.array([1.0, 0.35 + 0.2j, 0.15 - 0.1j, 0.05j], dtype=np.complex64)     # the 4 taps of tests/test_comb_sta.py
TAPS /= np.linalg.norm(TAPS)

OPS = ((20e6, 5.89e9), (20e6, 2.412e9), (10e6, 5.89e9))
DEFAULT_OP = OPS[0]
EQ_NAMES = ("LS", "LMS", "COMB", "STA")
N_BPSC = (1, 1, 2, 2, 4, 4, 6, 6)

# name: (encoding, PSDU bytes, SNR dB, frames per length, CFO bound or value, multipath, seed)
CASES = {
    "long_bpsk": (0, (1528,), 12.0, 8, 0.004, False, 11),
    "bpsk34": (1, (400,), 14.0, 12, 0.03, False, 12),
    "qpsk": (3, (150,), 21.0, 12, 0.03, True, 13),
    "qam16": (4, (700,), 20.0, 12, 0.004, True, 14),
    "qam64": (7, (1000,), 27.0, 12, 0.03, False, 15),
    "short": (2, (1, 3, 60), 25.0, 3, None, False, 16),           # CFO 0.005 on every frame
}

QUANTITIES = ("points", "llr", "llr_csi_rel", "csi_rel", "sym_stats_rel")
# 4 x the largest distance in profiles/independent_eq_distances.json, per quantity
TOL_Y = 4 * 1.556e-06           # measured 1.556e-06: max |Y - Y_ref| over the compared symbols, |Y| <~ 1.6; the unweighted LLRs
                                # (measured 1.32e-06, absolute) are held to it as well
TOL_LLR_CSI = 4 * 1.554e-06     # measured 1.554e-06: with llr_csi = 1, relative to max(|L_ref|, w) per carrier
TOL_CSI = 4 * 3.23e-07          # measured 3.23e-07: relative to max |H_ref| of the frame
TOL_STATS = 4 * 1.158e-06       # measured 1.158e-06: the sums of |y|, |y|^2, |y|^4 of a frame, relative
DELTA = 16 * 1.556e-06          # 16 x the measured point distance
TOL = dict(points=TOL_Y, llr=TOL_Y, llr_csi_rel=TOL_LLR_CSI, csi_rel=TOL_CSI, sym_stats_rel=TOL_STATS)
MIN_SHARE = 0.8                 # of the data symbols of the complete frames

_slots, _refs, _oracles = {}, {}, {}


def slots_of(name):
    """(iq [F, S] complex64, max_sym) of a case; frames of different lengths share one slot length"""
    if name not in _slots:
        enc, lengths, snr, per, cfo, multipath, seed = CASES[name]
        rng = np.random.default_rng(seed)
        # a PSDU below the 28 bytes of a MAC header and FCS is random bytes: the demodulator does not look inside
        txs = [txgen.encode_psdus(txgen.make_psdus(per, L, seed=seed * 100 + L) if L >= 28 else
                                  rng.integers(0, 256, (per, L), dtype=np.uint8), enc) for L in lengths]
        S = ((160 + max(t.samples.shape[1] for t in txs) + 320 + 63) // 64) * 64
        rows = []
        for k, t in enumerate(txs):
            c = np.full(per, 0.005) if cfo is None else rng.uniform(-cfo, cfo, per)
            rows.append(txgen.impair(t.samples, snr, cfo=c, lead=160, total=S, seed=seed * 1000 + k,
                                     taps=TAPS if multipath else None))
        _slots[name] = (np.concatenate(rows, axis=0), max(t.n_sym for t in txs))
    return _slots[name]


def reference(name, chan_est, op, rx_class=IndependentRx, cache=True):
    """the float64 receiver's outputs for a case; computed once per process for the unmutated class"""
    key = (name, chan_est, op)
    if cache and key in _refs:
        return _refs[key]
    iq, max_sym = slots_of(name)
    r = rx_class(bandwidth=op[0], frequency=op[1]).receive(iq, max_sym=max_sym, chan_est=chan_est)
    if cache:
        _refs[key] = r
    return r


def oracle_outputs(orc, name, chan_est, op):
    """the SPEC mode's outputs in the form `distances` takes: LLRs without and with the channel-state weight"""
    key = (name, chan_est, op)
    if key not in _oracles:
        iq, max_sym = slots_of(name)
        nb = N_BPSC[CASES[name][0]]
        run = {}
        for w in (0, 1):
            prm = orc.make_params(bandwidth=op[0], frequency=op[1], max_sym=max_sym, llr_bits=nb, chan_est=chan_est,
                                  llr_csi=w, math_mode=orc.MATH_SPEC)
            run[w] = orc.demod_batch(iq.reshape(-1), iq.shape[1], prm, want_eq=True, want_csi=True)
        a, b = run[0], run[1]
        assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["eq"], b["eq"])          # rule 12: signs do not change
        _oracles[key] = dict(frames=a["frames"], idx=a["idx"], eq=a["eq"], llr=a["llr"], llr_csi=b["llr"], csi=a["csi"],
                                sym_stats=orc.sym_stats(a["eq"], a["frames"]["n_sym_out"]))
    return _oracles[key]


def compared(ref, chan_est, delta):
    """(sym [F, max_sym] bool: symbols whose points / LLRs are compared, dec [F, max_sym, 48, 2] bool: components whose
    decisions are compared, whole [F] bool: frames with every symbol compared) -- from the reference alone"""
    F, max_sym = ref["eq"].shape[:2]
    n_sym = ref["n_sym"]
    have = ref["complete"][:, None] & (np.arange(max_sym)[None, :] < n_sym[:, None])
    m = np.full((F, max_sym, 48, 2), np.inf)
    m_sig = IndependentRx.margin(ref["eq_signal"], 1)
    for nb in (1, 2, 4, 6):
        sel = ref["complete"] & (ref["n_bpsc"] == nb)
        if sel.any():
            m[sel] = IndependentRx.margin(ref["eq"][sel], nb)
    safe = m >= delta
    sym = have.copy()
    if chan_est in (1, 3):
        risky = have & ~safe.all(axis=(2, 3))
        before = np.cumsum(risky, axis=1) - risky            # risky symbols in front of this one
        sym &= (before == 0) & (m_sig >= delta).all(axis=(1, 2))[:, None]
    dec = sym[:, :, None, None] & safe
    whole = ref["complete"] & (sym.sum(axis=1) == n_sym)
    return sym, dec, whole


def component_bits(idx, n_bpsc):
    """[..., 2] the bits of the real and of the imaginary axis of a decision"""
    h = max(n_bpsc // 2, 1)
    i = idx.astype(np.int64)
    re = i & ((1 << h) - 1)
    im = (i >> h) & ((1 << h) - 1) if n_bpsc > 1 else np.zeros_like(i)
    return np.stack([re, im], axis=-1)


def distances(ref, got, chan_est, delta=None):
    """`got`: dict(frames, idx, eq, llr, llr_csi, csi, sym_stats) of a float32 implementation (llr rows with
    llr_bits = n_bpsc).  Returns the largest distance per quantity, the share of compared symbols and the number of
    differing compared decisions; asserts the records."""
    delta = DELTA if delta is None else delta
    fr = got["frames"]
    F, max_sym = ref["eq"].shape[:2]
    cmp_ = ref["complete"]
    assert cmp_.all() and ((fr["flags"] & 8) != 0).all(), "all frames complete on both sides"
    for k in ("trigger", "frame_start", "encoding", "psdu_len", "n_sym"):
        assert np.array_equal(fr[k].astype(np.int64), ref[k].astype(np.int64)), k
    assert np.abs(fr["cfo_coarse"] - ref["cfo_coarse"]).max() < 1e-6, "cfo_coarse"
    assert np.abs(fr["cfo_fine"] - ref["cfo_fine"]).max() < 1e-6, "cfo_fine"
    assert np.abs(fr["snr_db"] - ref["snr_db"]).max() < 1e-3, "snr_db"
    nb = int(ref["n_bpsc"][0])
    assert (ref["n_bpsc"] == nb).all()
    sym, dec, whole = compared(ref, chan_est, delta)
    out = dict(share=float(sym.sum()) / float(ref["n_sym"].sum()), frames_whole=int(whole.sum()))
    out["points"] = float(np.abs(got["eq"].astype(np.complex128) - ref["eq"])[sym].max())
    L = got["llr"].reshape(F, max_sym, 48, nb).astype(np.float64)
    out["llr"] = float(np.abs(L - ref["llr"])[sym].max())
    Lw = got["llr_csi"].reshape(F, max_sym, 48, nb).astype(np.float64)
    scale = np.maximum(np.abs(ref["llr_w"]), ref["weight"][:, None, :, None])
    out["llr_csi_rel"] = float((np.abs(Lw - ref["llr_w"]) / scale)[sym].max())
    hmax = np.abs(ref["csi"]).max(axis=1)
    out["csi_rel"] = float((np.abs(got["csi"].astype(np.complex128) - ref["csi"]) / hmax[:, None]).max())
    st = got["sym_stats"][:, :3].astype(np.float64)
    out["sym_stats_rel"] = float((np.abs(st - ref["sym_stats"]) / ref["sym_stats"])[whole].max()) if whole.any() else None
    d = component_bits(got["idx"], nb) != component_bits(ref["idx"], nb)
    out["decisions"] = int(dec.sum())
    out["decisions_differ"] = int((d & dec).sum())
    return out


def check(out, what=""):
    """the assertions of a case x equaliser x operating point"""
    assert out["share"] >= MIN_SHARE, (what, out)
    assert out["frames_whole"] >= 1, (what, out)
    for q in QUANTITIES:
        assert out[q] <= TOL[q], (what, q, out)
    assert out["decisions_differ"] == 0, (what, out)
