"""The host-made records and decisions of tests/hard_rows.py, on the CPU: for every batch tests/test_gpu_hard_rows.py sends
to the device, the independent NumPy restatement of the hard decoder's rule (tests/hard_viterbi_ref.py: int64 metrics,
never normalised) decodes what the oracle's decode_mac decodes -- whole record arrays, whole PSDU rows --, so the
oracle is pinned from a second side on input that no transmission produces; the conditions that keep each batch from
passing vacuously hold (same table, same seeds); and the margins the byte metrics of decode_q_kernel rest on hold over
all of them."""
import numpy as np
import pytest

import hard_rows as hr
import hard_viterbi_ref as ref
import soft_rows as sr
import soft_viterbi_ref as sref


def test_frame_dtype_is_the_bindings_and_the_oracles():
    from oracle import oracle
    from wifirx import capi
    assert sr.FRAME_DTYPE == capi.FRAME_DTYPE == oracle.FRAME_DTYPE == hr.FRAME_DTYPE
    assert (sr.F_DETECTED, sr.F_SYNC, sr.F_SIGNAL, sref.F_COMPLETE, sref.F_LLR, sref.F_DECODED, sref.F_CRC_OK) == \
        (capi.F_DETECTED, capi.F_SYNC, capi.F_SIGNAL, capi.F_COMPLETE, capi.F_LLR, capi.F_DECODED, capi.F_CRC_OK) == \
        (oracle.F_DETECTED, oracle.F_SYNC, oracle.F_SIGNAL, oracle.F_COMPLETE, oracle.F_LLR, oracle.F_DECODED, oracle.F_CRC_OK)


def test_the_table_covers_what_the_issue_lists():
    assert set(hr.VALUE_SPECS + ("ladder",) + hr.UNIFORM_SPECS + hr.LONG_SPECS + hr.EDGE_SPECS + hr.N_SPECS) == set(hr.SPECS)
    assert {hr.SPECS[s].cls for s in hr.VALUE_SPECS} == {"coherent", "flips", "random", "zeros", "ones", "highbits"}
    assert {int(s.split("_")[1]) for s in hr.UNIFORM_SPECS} >= {0, 3, 5, 6}
    assert {hr.SPECS[s].cls for s in hr.LONG_SPECS} == {"flips", "random"} and len(hr.LONG_SPECS) == 16
    assert hr.N_SHAPES == (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
    assert (hr.BOUND_SPREAD, hr.BOUND_CAND_DIFF, hr.BOUND_GROWTH) == (12, 14, 96)


@pytest.mark.parametrize("name", sorted(hr.SPECS))
def test_reference_equals_the_oracle_and_the_batch_is_honest(name):
    """hard_viterbi_ref == orc.decode_batch: all records, and bytes 0 .. psdu_len - 1 of the decoded frames with zeros
    everywhere else in both; then the batch's honesty conditions, on the reference alone"""
    b, fr, psdu, info = hr.reference(name)
    _, ofr, opsdu = hr.oracle_reference(name)
    assert np.array_equal(fr, ofr), np.nonzero(fr != ofr)[0][:8]
    assert np.array_equal(psdu, opsdu), np.nonzero((psdu != opsdu).any(axis=1))[0][:8]
    keep = np.arange(b.spec.psdu_stride)[None, :] < np.where((fr["flags"] & sref.F_DECODED) != 0, fr["psdu_len"], 0)[:, None]
    assert not psdu[~keep].any() and not opsdu[~keep].any()
    print(name, hr.check_conditions(name))


def test_margins_of_the_byte_metrics():
    """what decode_q_kernel's comment derives, as conditions over every batch of the table: from step 6 on a frame's 64
    metrics lie within 12 of each other and the two candidates of a state within 14; the minimum grows by at most 96 in 48
    steps.  The figures recorded in hard_rows' docstring are the ones the table gives."""
    mg = ref.Margins()
    for name in sorted(hr.SPECS):
        m = hr.reference(name)[3]["margins"]
        print(name, "spread", m.spread, "cand_diff", m.cand_diff, "growth", m.growth)
        mg.merge(m)
    print("all", mg)
    assert mg.spread <= hr.BOUND_SPREAD and mg.cand_diff <= hr.BOUND_CAND_DIFF and mg.growth <= hr.BOUND_GROWTH
    assert (mg.spread, mg.cand_diff, mg.growth) == (hr.MEASURED_SPREAD, hr.MEASURED_CAND_DIFF, hr.MEASURED_GROWTH)


def test_high_bits_are_ignored_by_both():
    """bits at or above n_bpsc of a decision byte: same records and bytes from the reference and from the oracle"""
    (_, fr, psdu, _), (_, fr0, psdu0, _) = hr.reference("values_highbits"), hr.reference("values_coherent")
    assert np.array_equal(fr, fr0) and np.array_equal(psdu, psdu0)
    (_, ofr, opsdu), (_, ofr0, opsdu0) = hr.oracle_reference("values_highbits"), hr.oracle_reference("values_coherent")
    assert np.array_equal(ofr, ofr0) and np.array_equal(opsdu, opsdu0)


def test_planes_hold_the_bits_below_n_bpsc_only():
    """the bit planes of random decisions (garbage in every bit) are those of the same decisions with the high bits cleared"""
    b = hr.build("n_65")
    assert (b.idx & ~hr._nb_mask(b.recs)).any()
    assert np.array_equal(b.planes(), hr.planes_of(b.recs, b.idx & hr._nb_mask(b.recs), b.spec.max_sym))
    assert b.planes().shape == (65, b.spec.max_sym * 12) and b.planes().any()
