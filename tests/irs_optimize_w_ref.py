"""NUMERICS.md rule 31 restated on the host: what wifirx_irs_optimize_weighted (wr_irs_optimize.hip) computes, value for value.

Rule 31 is rule 30 with a float32 weight w_rho on every row: tw_rho = (w_rho t.re, w_rho t.im) behind rule 30's product t_rho (one
multiply per part, no fma), w_rho q_rho behind rule 30's q_rho, and a row with w_rho == 0 (either sign) contributes +0 to both
sums: selected, not multiplied.  The lane pairing, the butterfly (`fold`), the argmax and the start codes are tests/irs_optimize_ref.py's
own, imported.  With `weights=None` `optimize` returns irs_optimize_ref.optimize's result itself.  `direct()` is the same
algorithm in float64 with plain sums: the definition the rule's bounds refer to.

`mutant` switches one deliberate mistake on, for tests/test_irs_optimize_w_ref.py's mutation tests: "dropped" (the weights are
ignored in z), "abs" (|w| is used), "power" (the power trace is unweighted), "zero_kept" (a zero weight multiplies instead of
selecting +0), "upper" (the rows 64 and above take the weights of the rows i instead of i + 64), "sets" (per-set weights all read
block 0)."""
import numpy as np

import irs_optimize_ref as orf
import irs_ref
from irs_optimize_ref import START_GIVEN, START_REF, START_ZERO, argmax, fold, start_codes  # noqa: F401 (re-exported)
from wifirx import irs

F32 = np.float32
MUTANTS = ("dropped", "abs", "power", "zero_kept", "upper", "sets")


def weigh(w, v, mutant=None):
    """w_rho v_rho in float32, +0 where w_rho == 0: float32 [R]"""
    if mutant == "zero_kept":
        return w * v
    return np.where(w != 0, w * v, F32(0)).astype(F32)


def row_w(weights, R, mutant=None):
    """the weights one set works with: float32 [R]"""
    w = np.asarray(weights, dtype=F32).reshape(R).copy()
    if mutant == "abs":
        w = np.abs(w)
    if mutant == "upper" and R > 64:
        w[64:] = w[:R - 64]
    return w


def optimize_set(q, weights, bits, max_sweeps, start=START_REF, blocked=False, codes_in=None, mutant=None, trace=None,
                 early_exit=True):
    """one set: q complex64 [R, J], weights float32 [R] -> (codes uint8 [G], power float32 [max_sweeps + 1], sweeps).  trace: a
    list that receives (g, c_old, c_new) of every step.  early_exit=False runs every sweep (rule 30's step 5: no bit changes)"""
    q = np.asarray(q, dtype=np.complex64)
    R, J = q.shape
    G, up = J - 1, 3 - bits
    w = row_w(weights, R, mutant)
    ones = np.ones(R, F32)
    wz, wp = (ones if mutant == "dropped" else w), (ones if mutant == "power" else w)
    re, im = irs_ref.parts(q)
    er, ei = re[:, 1:], im[:, 1:]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        codes = start_codes(q, bits, start, blocked, codes_in).copy()     # rule 29's decision on row 0, whatever w_0 is
        sr, si = (np.zeros(R, F32), np.zeros(R, F32)) if blocked else (re[:, 0].copy(), im[:, 0].copy())
        for g in range(G):
            k = int(codes[g]) << up
            pr, pi = irs_ref.mul((er[:, g], ei[:, g]), (irs.PHASES_RE[k], irs.PHASES_IM[k]))
            sr, si = sr + pr, si + pi
        pw = lambda: fold(weigh(wp, sr * sr + si * si, mutant))
        power = np.empty(max_sweeps + 1, F32)
        power[0] = pw()
        sweeps = 0
        for it in range(1, max_sweeps + 1):
            changed = False
            for g in range(G):
                e = (er[:, g], ei[:, g])
                k = int(codes[g]) << up
                pr, pi = irs_ref.mul(e, (irs.PHASES_RE[k], irs.PHASES_IM[k]))
                rr, ri = sr - pr, si - pi
                tr, ti = irs_ref.mul((rr, -ri), e)
                c_new = argmax(fold(weigh(wz, tr, mutant)), fold(weigh(wz, ti, mutant)), bits)
                if trace is not None:
                    trace.append((g, int(codes[g]), c_new))
                if c_new != codes[g]:
                    k = c_new << up
                    nr, ni = irs_ref.mul(e, (irs.PHASES_RE[k], irs.PHASES_IM[k]))
                    sr, si = rr + nr, ri + ni
                    codes[g] = c_new
                    changed = True
            power[it] = pw()
            if not changed and early_exit:
                power[it:] = power[it]
                break
            sweeps += changed
    return codes, power, sweeps


def optimize(coef, bits, max_sweeps, start=START_REF, blocked=False, codes_in=None, group=None, n_elems=None, weights=None,
             mutant=None):
    """wifirx_irs_optimize_weighted restated: coef complex64 [n_sets, R, J], weights float32 [R] or [n_weight_sets, R] with
    n_weight_sets 1 or n_sets (set r reads block r % n_weight_sets).  Returns irs_optimize_ref.optimize's dict"""
    if weights is None:
        return orf.optimize(coef, bits, max_sweeps, start, blocked, codes_in, group, n_elems)
    q = np.asarray(coef, dtype=np.complex64)
    q = q[None] if q.ndim == 2 else q
    n_sets, R, J = q.shape
    G = J - 1
    w = np.asarray(weights, dtype=F32).reshape(-1, R)
    assert w.shape[0] in (1, n_sets)
    gm = np.arange(G if n_elems is None else n_elems) if group is None else np.asarray(group).reshape(-1).astype(np.intp)
    codes, power, sweeps = np.empty((n_sets, G), np.uint8), np.empty((n_sets, max_sweeps + 1), F32), np.empty(n_sets, np.uint8)
    for r in range(n_sets):
        ci = None if codes_in is None else np.asarray(codes_in).reshape(n_sets, G)[r]
        wr = w[0 if mutant == "sets" else r % w.shape[0]]
        codes[r], power[r], sweeps[r] = optimize_set(q[r], wr, bits, max_sweeps, start, blocked, ci, mutant)
    psi = irs.PHASES[codes[:, gm].astype(np.intp) << (3 - bits)]
    return {"codes": codes, "psi": psi, "power": power, "sweeps": sweeps}


def used(weights, x):
    """the rows the rule's sums see: (weights float64 [R'], x [R', ...]) for x [R, ...], the rows of weight 0 taken out"""
    w = np.asarray(weights, np.float64).reshape(-1)
    keep = w != 0
    return w[keep], np.asarray(x)[keep]


def true_power(q, weights, codes, bits, blocked=False):
    """P_w of the definition in float64 for given codes, one set: q [R, J], codes [G] -> float"""
    w, qd = used(weights, np.asarray(q, dtype=np.complex128))
    ph = irs.PHASES.astype(np.complex128)[np.asarray(codes).reshape(-1).astype(np.intp) << (3 - bits)]
    s = (qd[:, 1:] * ph[None, :]).sum(axis=-1) + (0 if blocked else qd[:, 0])
    return float((w * np.abs(s) ** 2).sum())


def direct(q, weights, bits, max_sweeps, start=START_REF, blocked=False, codes_in=None):
    """the same algorithm in float64 for one set (plain sums, the state recomputed from the codes at every step, the rows of
    weight 0 absent): returns (codes, power float64 [max_sweeps + 1], sweeps).  The start codes are the float32 rule's"""
    q32 = np.asarray(q, dtype=np.complex64)
    w, qd = used(weights, q32.astype(np.complex128))
    G, up = q32.shape[1] - 1, 3 - bits
    ph = irs.PHASES.astype(np.complex128)
    codes = start_codes(q32, bits, start, blocked, codes_in).copy()
    d = np.zeros(qd.shape[0], np.complex128) if blocked else qd[:, 0]
    e = qd[:, 1:]
    total = lambda: d + (e * ph[codes.astype(np.intp) << up][None, :]).sum(axis=1)
    p_w = lambda: (w * np.abs(total()) ** 2).sum()
    power = np.empty(max_sweeps + 1)
    power[0] = p_w()
    sweeps = 0
    for it in range(1, max_sweeps + 1):
        changed = False
        s = total()
        for g in range(G):
            r = s - e[:, g] * ph[int(codes[g]) << up]
            z = (w * np.conj(r) * e[:, g]).sum()
            m = (z * ph[np.arange(1 << bits) << up]).real
            c_new = int(np.argmax(m))                              # the first maximum: the lowest c
            if c_new != codes[g]:
                s = r + e[:, g] * ph[c_new << up]
                codes[g] = c_new
                changed = True
        power[it] = p_w()
        if not changed:
            power[it:] = power[it]
            break
        sweeps += 1
    return codes, power, sweeps


def power_bound(q, weights, max_sweeps, blocked=False):
    """rule 31's bound on |power - P_w| under the same codes, one set: rule 30's (b) with |w_rho| inside the sum over the rows and
    one more rounding for the weighted term: (2 state_terms + 10) 2^-24 sum_rho |w_rho| A_rho^2"""
    w, qd = used(weights, np.asarray(q, dtype=np.complex128))
    a = orf.row_weight(qd, blocked)
    G = np.shape(q)[-1] - 1
    return float((2 * orf.state_terms(G, max_sweeps) + 10) * 2.0 ** -24 * (np.abs(w) * a * a).sum())


def decision_allowance(q, weights, max_sweeps, blocked=False):
    """rule 31's allowance per update, one set: rule 30's (c) with |w_rho| inside the sums over the rows and one more rounding
    per weighted term: 4 2^-24 (R + 8 + state_terms) max_g sum_rho |w_rho| A_rho |e_{rho,g}|; R counts every row of the call"""
    R, G = np.shape(q)[-2], np.shape(q)[-1] - 1
    w, qd = used(weights, np.asarray(q, dtype=np.complex128))
    a = orf.row_weight(qd, blocked)
    worst = ((np.abs(w) * a)[:, None] * np.abs(qd[:, 1:])).sum(axis=0).max() if w.size else 0.0
    return float(4 * 2.0 ** -24 * (R + 8 + orf.state_terms(G, max_sweeps)) * worst)
