"""Host-built input rows for the receive-diversity combiner (NUMERICS.md rule 23): the batches that tests/test_diversity_ref.py
runs through the reference and tests/test_gpu_diversity.py through the device, and the comparison they share.  No demod:
records, points and channel estimates are drawn, so that every clause of the rule is met on purpose."""
import numpy as np

import diversity_ref as dr
from wifirx import capi

N_SLOTS, MAX_SYM, LLR_BITS = 37, 7, 6
N_ANT = (1, 2, 3, 8)
CASES = ("all_usable", "no_signal", "no_complete", "other_encoding", "other_psdu_len", "none_usable", "equal_snr", "nan_snr",
         "zero_csi", "inf_csi")
GOOD = capi.F_DETECTED | capi.F_SYNC | capi.F_SIGNAL | capi.F_COMPLETE


def gains(n_ant):
    """inverse noise powers: distinct, one of them 0 from three antennas on (an antenna switched off by its weight)"""
    g = (0.5 + 0.375 * np.arange(n_ant)).astype(np.float32)
    if n_ant >= 3:
        g[1] = 0.0
    return g


def build(case, n_ant, seed=0, n_slots=N_SLOTS, max_sym=MAX_SYM):
    """(frames [A][n], carrier [A][n, max_sym, 48], csi [A][n, 52]) of a case.  Every slot draws an encoding 0..7 and n_sym
    1..max_sym; the antenna that a case singles out moves with the slot, so it is the first, a middle and the last one in turn."""
    rng = np.random.default_rng([seed, CASES.index(case), n_ant])
    enc = rng.integers(0, 8, n_slots)
    n_sym = rng.integers(1, max_sym + 1, n_slots)
    plen = rng.integers(1, 1500, n_slots)
    frames, carrier, csi = [], [], []
    for a in range(n_ant):
        f = np.zeros(n_slots, capi.FRAME_DTYPE)
        # (LLR / DECODED / CRC_OK set on some inputs: the combiner has to clear them)
        f["flags"] = GOOD | np.where(rng.random(n_slots) < 0.5, capi.F_LLR | capi.F_DECODED | capi.F_CRC_OK, 0)
        f["trigger"], f["frame_start"] = 100 + a, 64 + a
        f["cfo_coarse"], f["cfo_fine"] = rng.normal(0, 0.01, n_slots), rng.normal(0, 0.001, n_slots)
        f["snr_db"] = rng.uniform(0, 30, n_slots)
        f["psdu_len"], f["encoding"], f["n_bpsc"] = plen, enc, np.take(dr.N_BPSC, enc)
        f["n_sym"] = f["n_sym_out"] = n_sym
        frames.append(f)
        carrier.append((rng.normal(0, 0.7, (n_slots, max_sym, 48)) + 1j * rng.normal(0, 0.7, (n_slots, max_sym, 48))).astype(np.complex64))
        csi.append((rng.normal(0, 1, (n_slots, 52)) + 1j * rng.normal(0, 1, (n_slots, 52))).astype(np.complex64))
    odd = np.arange(n_slots) % n_ant                    # the antenna singled out in slot i
    for i in range(n_slots):
        f = frames[odd[i]]
        if case == "no_signal":
            f["flags"][i] &= ~np.uint32(capi.F_SIGNAL)
        elif case == "no_complete":
            f["flags"][i] &= ~np.uint32(capi.F_COMPLETE)
        elif case == "other_encoding":
            f["encoding"][i] = (enc[i] + 1 + i % 7) % 8
            f["n_bpsc"][i] = dr.N_BPSC[f["encoding"][i]]
            f["n_sym"][i] = f["n_sym_out"][i] = 1 + (n_sym[i] + i) % max_sym
        elif case == "other_psdu_len":
            f["psdu_len"][i] = plen[i] + 1
        elif case == "none_usable" and i % 3 != 1:
            for a in range(n_ant):
                frames[a]["flags"][i] &= ~np.uint32(capi.F_SIGNAL if (i + a) % 2 else capi.F_COMPLETE)
        elif case == "equal_snr":
            for a in range(n_ant):
                frames[a]["snr_db"][i] = frames[0]["snr_db"][i] if i % 2 else max(fr["snr_db"][i] for fr in frames)
        elif case == "nan_snr":
            f["snr_db"][i] = np.nan
        elif case == "zero_csi":
            for a in range(n_ant):
                csi[a][i, dr.OCC[i % 48]] = 0
                if i % 2:
                    csi[a][i, dr.OCC[(i + 5) % 48]] = -0.0
        elif case == "inf_csi":
            csi[odd[i]][i, dr.OCC[(3 * i) % 48]] = np.inf if i % 2 else complex(1.0, -np.inf)
            if i % 5 == 0:
                csi[odd[i]][i, dr.OCC[(3 * i + 7) % 48]] = complex(np.nan, 0.5)
    return frames, carrier, csi


def same_bits(a, b):
    """bit-equal arrays of one dtype, except that in float arrays (float32, complex64) any NaN matches any NaN: the payload and
    sign of a NaN that an operation makes differ between processors"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype in (np.dtype(np.float32), np.dtype(np.complex64)):
        fa, fb = a.view(np.float32), b.view(np.float32)
        na, nb = np.isnan(fa), np.isnan(fb)
        return bool(np.array_equal(na, nb)) and bool(np.array_equal(fa.view(np.uint32)[~na], fb.view(np.uint32)[~nb]))
    return bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def same_outputs(got, want, bf16):
    """names of the outputs of `got` that differ from `want` (dicts of new_outputs arrays)"""
    from llr_bf16_ref import same_bf16
    bad = []
    for k in ("frames", "idx", "llr", "carrier", "used_mask"):
        if want.get(k) is None:
            continue
        ok = same_bf16(got[k], want[k]) if (k == "llr" and bf16) else same_bits(got[k], want[k])
        if not ok:
            bad.append(k)
    return bad
