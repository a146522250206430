"""NUMERICS.md rule 30 restated on the host: what wifirx_irs_optimize (wr_irs_optimize.hip) computes, value for value.

NumPy float32 on separate real and imaginary parts, rule 17's plain ch_mul / ch_add (tests/irs_ref.py's `mul`), the lane pairing
(lane i forms the values of the rows i and i + 64, absent rows +0), rule 25's butterfly and rule 25's argmax
(wifirx.irs.align_codes).  `direct()` is the same algorithm in float64 with plain sums: the definition the rule's bounds refer to.

`mutant` switches one deliberate mistake on, for tests/test_irs_optimize_ref.py's mutation tests: "own" (the group's own term is not
removed: z is formed from s, not from r), "conj" (z = sum r e, not conj(r) e), "state" (s is not updated when a code changes),
"tie" (the argmax takes a later c on a tie: >=), "blocked" (column 0 is read although the direct path is blocked), "rows" (the rows
64 and above are dropped from the sums)."""
import numpy as np

import irs_ref
from wifirx import irs

F32 = np.float32
START_REF, START_GIVEN, START_ZERO = 0, 1, 2
MUTANTS = ("own", "conj", "state", "tie", "blocked", "rows")
LANES = np.arange(64)


def fold(v, mutant=None):
    """the rule's sum over the rows: v float32 [R], R <= 128 -> one float32.  Lane i forms v_i + v_{i+64} (absent rows are +0),
    then the butterfly over lane xor 32, 16, 8, 4, 2, 1"""
    pad = np.zeros(128, F32)
    pad[:v.size] = v
    if mutant == "rows":
        pad[64:] = 0
    acc = pad[:64] + pad[64:]
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[LANES ^ m]
    return acc[0]


def argmax(zr, zi, bits, mutant=None):
    """rule 25's argmax on Re(ch_mul(z, C_c)): ascending c, strict >, the lowest c wins a tie, a NaN never replaces the maximum"""
    if mutant != "tie":
        return int(irs.align_codes(F32(zr), F32(zi), 0, 0, bits))
    up, best = 3 - bits, 0
    top = zr * irs.PHASES_RE[0] - zi * irs.PHASES_IM[0]
    for c in range(1, 1 << bits):
        m = zr * irs.PHASES_RE[c << up] - zi * irs.PHASES_IM[c << up]
        if m >= top:
            top, best = m, c
    return best


def start_codes(q, bits, start, blocked, codes_in=None):
    """step 1 for one set: q complex64 [R, J] -> uint8 [G]"""
    G = q.shape[1] - 1
    if start == START_ZERO:
        return np.zeros(G, np.uint8)
    if start == START_GIVEN:
        return (np.asarray(codes_in, np.uint8).reshape(G) & np.uint8((1 << bits) - 1)).astype(np.uint8)
    re, im = irs_ref.parts(q[0])
    hd = (F32(0), F32(0)) if blocked else (re[0], im[0])
    return irs.align_codes(re[1:], im[1:], hd[0], hd[1], bits)


def optimize_set(q, bits, max_sweeps, start=START_REF, blocked=False, codes_in=None, mutant=None, trace=None, early_exit=True):
    """one set: q complex64 [R, J] -> (codes uint8 [G], power float32 [max_sweeps + 1], sweeps).  trace: a list that receives
    (g, c_old, c_new) of every step, for the float64 shadow of tests/test_irs_optimize_ref.py.  early_exit=False runs every sweep
    (step 5 says that this changes no bit)"""
    q = np.asarray(q, dtype=np.complex64)
    R, J = q.shape
    G, up = J - 1, 3 - bits
    re, im = irs_ref.parts(q)
    er, ei = re[:, 1:], im[:, 1:]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        codes = start_codes(q, bits, start, blocked, codes_in).copy()
        if blocked and mutant != "blocked":
            sr, si = np.zeros(R, F32), np.zeros(R, F32)
        else:
            sr, si = re[:, 0].copy(), im[:, 0].copy()
        for g in range(G):
            k = int(codes[g]) << up
            pr, pi = irs_ref.mul((er[:, g], ei[:, g]), (irs.PHASES_RE[k], irs.PHASES_IM[k]))
            sr, si = sr + pr, si + pi
        power = np.empty(max_sweeps + 1, F32)
        power[0] = fold(sr * sr + si * si, mutant)
        sweeps = 0
        for it in range(1, max_sweeps + 1):
            changed = False
            for g in range(G):
                e = (er[:, g], ei[:, g])
                k = int(codes[g]) << up
                pr, pi = irs_ref.mul(e, (irs.PHASES_RE[k], irs.PHASES_IM[k]))
                rr, ri = (sr, si) if mutant == "own" else (sr - pr, si - pi)
                tr, ti = irs_ref.mul((rr, ri if mutant == "conj" else -ri), e)
                c_new = argmax(fold(tr, mutant), fold(ti, mutant), bits, mutant)
                if trace is not None:
                    trace.append((g, int(codes[g]), c_new))
                if c_new != codes[g]:
                    k = c_new << up
                    nr, ni = irs_ref.mul(e, (irs.PHASES_RE[k], irs.PHASES_IM[k]))
                    if mutant != "state":
                        sr, si = (sr - pr) + nr, (si - pi) + ni
                    codes[g] = c_new
                    changed = True
            power[it] = fold(sr * sr + si * si, mutant)
            if not changed and early_exit:                        # every later sweep would repeat this one bit for bit
                power[it:] = power[it]
                break
            sweeps += changed
    return codes, power, sweeps


def optimize(coef, bits, max_sweeps, start=START_REF, blocked=False, codes_in=None, group=None, n_elems=None, mutant=None):
    """wifirx_irs_optimize restated: coef complex64 [n_sets, R, J].  Returns a dict: codes uint8 [n_sets, G], psi complex64
    [n_sets, N], power float32 [n_sets, max_sweeps + 1], sweeps uint8 [n_sets]"""
    q = np.asarray(coef, dtype=np.complex64)
    q = q[None] if q.ndim == 2 else q
    n_sets, R, J = q.shape
    G = J - 1
    gm = np.arange(G if n_elems is None else n_elems) if group is None else np.asarray(group).reshape(-1).astype(np.intp)
    codes, power, sweeps = np.empty((n_sets, G), np.uint8), np.empty((n_sets, max_sweeps + 1), F32), np.empty(n_sets, np.uint8)
    for r in range(n_sets):
        ci = None if codes_in is None else np.asarray(codes_in).reshape(n_sets, G)[r]
        codes[r], power[r], sweeps[r] = optimize_set(q[r], bits, max_sweeps, start, blocked, ci, mutant)
    psi = irs.PHASES[codes[:, gm].astype(np.intp) << (3 - bits)]
    return {"codes": codes, "psi": psi, "power": power, "sweeps": sweeps}


def true_power(q, codes, bits, blocked=False):
    """P of the definition in float64 for given codes: q [n_sets, R, J], codes [n_sets, G] -> float64 [n_sets]"""
    q = np.asarray(q, dtype=np.complex128)
    q = q[None] if q.ndim == 2 else q
    ph = irs.PHASES.astype(np.complex128)[np.asarray(codes).reshape(q.shape[0], -1).astype(np.intp) << (3 - bits)]
    s = (q[:, :, 1:] * ph[:, None, :]).sum(axis=-1) + (0 if blocked else q[:, :, 0])
    return (np.abs(s) ** 2).sum(axis=-1)


def direct(q, bits, max_sweeps, start=START_REF, blocked=False, codes_in=None):
    """the same algorithm in float64 for one set (plain sums, the state recomputed from the codes at every step): returns (codes,
    power float64 [max_sweeps + 1], sweeps).  The start codes are the float32 rule's (they are an input of the ascent)."""
    q32 = np.asarray(q, dtype=np.complex64)
    qd = q32.astype(np.complex128)
    G, up = qd.shape[1] - 1, 3 - bits
    ph = irs.PHASES.astype(np.complex128)
    codes = start_codes(q32, bits, start, blocked, codes_in).copy()
    d = np.zeros(qd.shape[0], np.complex128) if blocked else qd[:, 0]
    e = qd[:, 1:]
    power = np.empty(max_sweeps + 1)
    total = lambda: d + (e * ph[codes.astype(np.intp) << up][None, :]).sum(axis=1)
    power[0] = (np.abs(total()) ** 2).sum()
    sweeps = 0
    for it in range(1, max_sweeps + 1):
        changed = False
        s = total()
        for g in range(G):
            r = s - e[:, g] * ph[int(codes[g]) << up]
            z = (np.conj(r) * e[:, g]).sum()
            m = (z * ph[np.arange(1 << bits) << up]).real
            c_new = int(np.argmax(m))                              # the first maximum: the lowest c
            if c_new != codes[g]:
                s = r + e[:, g] * ph[c_new << up]
                codes[g] = c_new
                changed = True
        power[it] = (np.abs(total()) ** 2).sum()
        if not changed:
            power[it:] = power[it]
            break
        sweeps += 1
    return codes, power, sweeps


def row_weight(q, blocked=False):
    """A_rho = |d_rho| + sum_g |e_{rho,g}|: no state of the row, under any codes, is longer (|C_c| = 1); float64 [..., R]"""
    q = np.asarray(q, dtype=np.complex128)
    a = np.abs(q[..., 1:]).sum(axis=-1)
    return a if blocked else a + np.abs(q[..., 0])


def state_terms(G, max_sweeps):
    """rule 30's count of roundings behind a state s_rho, in units of 2^-24 A_rho, to first order: G + 2 for the G adds of step 2
    and their products, 4 for every update (two adds and the new product; the product taken out is the one put in, bit for bit),
    at most U = G max_sweeps updates, times 1.5 >= sqrt(2) for the two parts"""
    return 1.5 * (G + 4 * G * max_sweeps + 2)


def power_bound(q, max_sweeps, blocked=False):
    """rule 30's bound on |power - P| for P the float64 definition under the same codes: 2 |s| ds over the rows, 2 roundings of
    q_rho and the 7 adds of the lane pair and the butterfly: (2 state_terms + 9) 2^-24 sum_rho A_rho^2; float64 [...]"""
    a = row_weight(q, blocked)
    G = np.shape(q)[-1] - 1
    return (2 * state_terms(G, max_sweeps) + 9) * 2.0 ** -24 * (a * a).sum(axis=-1)


def decision_allowance(q, max_sweeps, blocked=False):
    """rule 30's allowance per update: the float32 z differs from the float64 z of the codes in force by at most
    dz = 2^-24 ((R + 7) sum_rho |r_rho| |e_rho| + state_terms sum_rho A_rho |e_rho|) (the first term the roundings of t, the lane
    pair and the butterfly, the second the state's own distance), and a decision taken on it can lower the true power by
    4 dz at most.  With |r_rho| <= A_rho and the largest group: 4 2^-24 (R + 7 + state_terms) max_g sum_rho A_rho |e_{rho,g}|"""
    qd = np.asarray(q, dtype=np.complex128)
    R, G = qd.shape[-2], qd.shape[-1] - 1
    a = row_weight(qd, blocked)
    worst = (a[..., None] * np.abs(qd[..., 1:])).sum(axis=-2).max(axis=-1)
    return 4 * 2.0 ** -24 * (R + 7 + state_terms(G, max_sweeps)) * worst
