"""NUMERICS.md rule 23 restated on the host: what wifirx_diversity_combine (wr_diversity.hip) computes, value for value, in
NumPy float32 -- the reference antenna, the contributing set, the weights of rule 12 and their normalisation, the combined
points, and from them the decisions and LLRs of rule 7 (rule 15 for bf16 rows).  `direct()` is the textbook statement of
maximal-ratio combining in float64, sum w Y / sum w, that tests/test_diversity_ref.py holds this module against.

`mutant` switches one clause of the rule to a plausible wrong reading; every one of them must fail a named test
(profiles/diversity_mutations.txt)."""
import numpy as np

from detect_ref import fma32
from llr_bf16_ref import bf16_rne

F32 = np.float32
MRC, SELECT = 0, 1
F_SIGNAL, F_COMPLETE, F_LLR, F_DECODED, F_CRC_OK = 4, 8, 16, 32, 64
N_BPSC = (1, 1, 2, 2, 4, 4, 6, 6)
# the slicer thresholds 2a (16-QAM) and 2a, 4a, 6a (64-QAM) as the float32 values of include/wifirx_tables.h
T16_2 = F32(float.fromhex("0x1.43d136p-1"))
T64_2, T64_4, T64_6 = (F32(float.fromhex(h)) for h in ("0x1.3c0366p-2", "0x1.3c0366p-1", "0x1.da0518p-1"))
# occupied index (0..51) of data carrier k = 0..47: the pilots sit at 5, 19, 32 and 46
OCC = np.array([o for o in range(52) if o not in (5, 19, 32, 46)])
MUTANTS = ("tie_takes_later", "nan_replaces", "ignore_psdu_len", "no_zero_fallback", "gain_after_normalising")


def decide(y, n_bpsc):
    """the slicer of rule 7 on float32 points: bit k of the byte = coded bit k"""
    re, im = y.real.astype(F32), y.imag.astype(F32)
    are, aim = np.abs(re), np.abs(im)
    if n_bpsc == 1:
        r = (re > 0).astype(np.uint8)
    elif n_bpsc == 2:
        r = (re > 0) | ((im > 0) << 1)
    elif n_bpsc == 4:
        r = (re > 0) | ((are < T16_2) << 1) | ((im > 0) << 2) | ((aim < T16_2) << 3)
    else:
        r = ((re > 0) | ((are < T64_4) << 1) | (((are < T64_6) & (are > T64_2)) << 2) |
             ((im > 0) << 3) | ((aim < T64_4) << 4) | (((aim < T64_6) & (aim > T64_2)) << 5))
    return r.astype(np.uint8)


def llr(y, n_bpsc):
    """rule 7's LLRs of float32 points: [..., n_bpsc], the bits of the real axis first"""
    re, im = y.real.astype(F32), y.imag.astype(F32)
    are, aim = np.abs(re), np.abs(im)
    if n_bpsc == 1:
        v = [re]
    elif n_bpsc == 2:
        v = [re, im]
    elif n_bpsc == 4:
        v = [re, T16_2 - are, im, T16_2 - aim]
    else:
        v = [re, T64_4 - are, T64_2 - np.abs(are - T64_4), im, T64_4 - aim, T64_2 - np.abs(aim - T64_4)]
    return np.stack(v, axis=-1).astype(F32)


def weight(H):
    """rule 12: fma(H.im, H.im, H.re H.re) of complex64 estimates"""
    re, im = H.real.astype(F32), H.imag.astype(F32)
    return fma32(im, im, re * re)


def select(frames, max_sym, mode=MRC, mutant=None):
    """(r, C) of one slot: frames = the A records of the slot.  r = -1 and C = [] when no antenna is usable."""
    both = F_SIGNAL | F_COMPLETE
    usable = [a for a, f in enumerate(frames)
              if (int(f["flags"]) & both) == both and int(f["encoding"]) <= 7 and int(f["n_sym"]) <= max_sym]
    if not usable:
        return -1, []
    r = usable[0]
    for a in usable[1:]:
        s, best = F32(frames[a]["snr_db"]), F32(frames[r]["snr_db"])
        if mutant == "tie_takes_later":
            take = s >= best
        elif mutant == "nan_replaces":
            take = not (s <= best)
        else:
            take = s > best
        if take:
            r = a
    same = lambda a: frames[a]["encoding"] == frames[r]["encoding"] and \
        (mutant == "ignore_psdu_len" or frames[a]["psdu_len"] == frames[r]["psdu_len"])
    C = [r] if mode == SELECT else [a for a in usable if same(a)]
    return r, C


def combine_slot(Y, H, r, C, ant_gain=None, mutant=None):
    """The points of one slot: Y [A][n_sym, 48] complex64, H [A][52] complex64 -> (Y complex64 [n_sym, 48], W_eff float32 [48])"""
    w = {}
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a in C:
            w[a] = weight(H[a][OCC])
            if ant_gain is not None and mutant != "gain_after_normalising":
                w[a] = w[a] * F32(ant_gain[a])
        W = w[C[0]]
        for a in C[1:]:
            W = W + w[a]
        if mutant == "no_zero_fallback":
            fb = ~np.isfinite(W)
        else:
            fb = ~(np.isfinite(W) & (W > 0))
        if len(C) == 1:
            fb = np.ones(48, bool)
        re = im = None
        for a in C:
            u = (w[a] / W).astype(F32)
            if ant_gain is not None and mutant == "gain_after_normalising":
                u = u * F32(ant_gain[a])
            yre, yim = Y[a].real.astype(F32), Y[a].imag.astype(F32)
            if re is None:
                re, im = u * yre, u * yim
            else:
                re, im = fma32(u, yre, re), fma32(u, yim, im)
    out = np.where(fb, Y[r], (re + 1j * im).astype(np.complex64)).astype(np.complex64)
    # a copy bit for bit: np.where on complex64 keeps the payload of Y[r]
    return out, np.where(fb, w[r], W).astype(F32)


def new_outputs(n_slots, max_sym, llr_bits, bf16=False, fill=0xA5):
    """output arrays filled with a sentinel byte: frames, idx, llr, carrier, used_mask"""
    from wifirx import capi
    b = lambda dt, shape: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, fill, np.uint8).view(dt).reshape(shape)
    return dict(frames=b(capi.FRAME_DTYPE, (n_slots,)), idx=b(np.uint8, (n_slots, max_sym, 48)),
                llr=b(np.uint16 if bf16 else F32, (n_slots, max_sym * 48 * llr_bits)) if llr_bits else None,
                carrier=b(np.complex64, (n_slots, max_sym, 48)), used_mask=b(np.uint8, (n_slots,)))


def combine(frames, carrier, csi, max_sym, llr_bits, out, mode=MRC, ant_gain=None, llr_csi=False, bf16=False, mutant=None):
    """wifirx_diversity_combine: frames [A][n] records, carrier [A][n, max_sym, 48] complex64, csi [A][n, 52] complex64; writes
    into the arrays of `out` (new_outputs; an entry that is None is not produced) what the rule writes and nothing else."""
    A, n = len(frames), len(frames[0])
    g = None if ant_gain is None else np.asarray(ant_gain, dtype=F32)
    for i in range(n):
        recs = [frames[a][i] for a in range(A)]
        r, C = select(recs, max_sym, mode, mutant)
        if r < 0:
            rec = recs[0].copy()
            rec["flags"] &= ~np.uint32(F_COMPLETE | F_LLR | F_DECODED | F_CRC_OK)
            out["frames"][i] = rec
            if out.get("used_mask") is not None:
                out["used_mask"][i] = 0
            continue
        rec = recs[r].copy()
        ns, nb = int(rec["n_sym"]), N_BPSC[int(rec["encoding"])]
        Y, Weff = combine_slot([carrier[a][i, :ns] for a in range(A)], [csi[a][i] for a in range(A)], r, C, g, mutant)
        if out.get("carrier") is not None:
            out["carrier"][i, :ns] = Y
        if out.get("idx") is not None:
            out["idx"][i, :ns] = decide(Y, nb)
        wrote = out.get("llr") is not None and nb <= llr_bits
        if wrote:
            with np.errstate(invalid="ignore", over="ignore"):
                L = llr(Y, nb)
                if llr_csi:
                    L = L * Weff[None, :, None]
            L = L.reshape(-1)
            out["llr"][i, :L.size] = bf16_rne(L) if bf16 else L
        rec["flags"] &= ~np.uint32(F_LLR | F_DECODED | F_CRC_OK)
        if wrote:
            rec["flags"] |= np.uint32(F_LLR)
        out["frames"][i] = rec
        if out.get("used_mask") is not None:
            out["used_mask"][i] = sum(1 << a for a in C)
    return out


def direct(Y, H, C, ant_gain=None):
    """maximal-ratio combining by its definition, in float64: sum_a w_a Y_a / sum_a w_a over the antennas of C, w_a = |H_a|^2 g_a.
    Y [A][n_sym, 48], H [A][52] -> complex128 [n_sym, 48]"""
    w = [np.abs(H[a][OCC].astype(np.complex128)) ** 2 * (1.0 if ant_gain is None else float(F32(ant_gain[a]))) for a in C]
    num = sum(wa[None, :] * Y[a].astype(np.complex128) for wa, a in zip(w, C))
    return num / sum(w)[None, :]
