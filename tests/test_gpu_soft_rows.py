"""wifirx_decode_batch_soft on the MI355X against tests/soft_viterbi_ref.py, bit for bit, on records and LLR rows made on
the host (tests/soft_rows.py) -- no demodulator in the loop, so the decoder's input space is the test's to steer: value
classes (noise, NaN / inf, zeros and -0, one magnitude, subnormals, sixty decades of range, magnitudes that overflow the
metrics), PSDU lengths 0 .. 1528, max_sym and psdu_stride edges, unaligned PSDU buffers, batch shapes around the 64
frames of a task, handles with narrow LLR rows, one to three waves serving sixteen tasks, failing scratch allocations,
and the rows the device's own demodulation writes for hostile samples.

Every comparison is over whole arrays: all frame records, and every byte of a PSDU buffer that was filled with 0xA5 and
sits between fences -- bytes 0 .. psdu_len - 1 of the decoded frames equal the reference, everything else still holds the
pattern.  float32 and bf16 rows (the reference reads the widened bf16 values).  The batches, their seeds and the
conditions that keep them honest are the table of tests/soft_rows.py, which tests/test_soft_rows.py runs on the CPU."""
import ctypes as C

import numpy as np
import pytest

import soft_rows as sr
import soft_viterbi_ref as ref
from helpers import Fenced
from llr_bf16_ref import bf16_to_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from wifirx import capi
    return capi


def soft_decode(capi, rx, d_frames, d_llr, ps, n):
    """wifirx_decode_batch_soft over device buffers; returns (rc, records, the whole PSDU allocation)"""
    out = capi.Out(d_frames.ptr, None, d_llr.ptr, None, ps.ptr, ps.stride, 1, None, None, None)
    rc = capi.lib().wifirx_decode_batch_soft(rx._h, n, C.byref(out))
    rx.sync()
    return rc, d_frames.download(capi.FRAME_DTYPE, n), ps.download()


def run_batch(capi, b, psdu_off=0, calls=1):
    """the batch through a handle of its own; one result per call (records and rows are uploaded afresh for each)"""
    sp = b.spec
    n = b.recs.size
    rx = capi.WifiRx(max_sym=sp.max_sym, llr_bits=sp.llr_bits, device=0, llr_format=b.fmt)
    res = []
    try:
        d_fr, d_llr = rx.alloc(n * 32), rx.alloc(b.rows.nbytes)
        ps = Fenced(rx, n, sp.psdu_stride, psdu_off)
        try:
            for _ in range(calls):
                d_fr.upload(b.recs)
                d_llr.upload(b.rows)
                ps.refill()
                res.append(soft_decode(capi, rx, d_fr, d_llr, ps, n))
        finally:
            for d in (d_fr, d_llr, ps):
                d.free()
    finally:
        rx.close()
    return ps, res


def assert_equals_reference(b, fr, psdu, ps, got):
    rc, frames, raw = got
    assert rc == 0
    assert np.array_equal(frames, fr), np.nonzero(frames != fr)[0][:8]
    want = ps.expected(sr.expected_psdu_buffer(b, fr, psdu))
    assert np.array_equal(raw, want), np.nonzero(raw != want)[0][:8] - ps.at


def check(capi, name, fmt, psdu_off=0):
    fig = sr.check_conditions(name, fmt)
    print(name, fmt, fig)
    b, fr, psdu, _ = sr.reference(name, fmt)
    ps, res = run_batch(capi, b, psdu_off)
    assert_equals_reference(b, fr, psdu, ps, res[0])
    return b, fr


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", sr.VALUE_SPECS)
def test_values(capi, name, fmt):
    """every value class x all eight rates in one batch, three lengths per rate (short frames end while their wave goes on)"""
    check(capi, name, fmt)


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", sr.LONG_SPECS)
def test_longest_frames(capi, name, fmt):
    """1528 bytes on a max_sym = 511 handle (12 264 .. 12 312 steps: the largest scratch slice, the longest trace-back); 1529
    bytes left alone"""
    b, fr = check(capi, name, fmt)
    assert (b.recs["psdu_len"] == ref.MAX_PSDU + 1).sum() == 1 and b.meant.sum() == 64


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", ("short", "maxsym"))
def test_lengths(capi, name, fmt):
    """psdu_len 0 .. 8 (no CRC_OK below 4, the tail loop of the finish); n_sym == max_sym decoded, max_sym + 1 left alone"""
    b, fr = check(capi, name, fmt)
    if name == "maxsym":
        assert (b.recs["n_sym"][b.meant] == b.spec.max_sym).all() and (b.recs["n_sym"][~b.meant] == b.spec.max_sym + 1).all()
        assert b.meant.any() and (~b.meant).any()
    else:
        assert set(b.recs["psdu_len"].tolist()) == {0, 1, 2, 3, 4, 5, 7, 8}
        assert not (fr["flags"][b.recs["psdu_len"] < 4] & ref.F_CRC_OK).any()


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_psdu_stride_and_alignment(capi, off, fmt):
    """psdu_len == psdu_stride (odd) decoded, psdu_stride + 1 left alone; the PSDU pointer 0 .. 3 bytes behind a 16-byte
    boundary (rows that are not dword aligned leave byte by byte)"""
    b, fr = check(capi, "stride", fmt, psdu_off=off)
    assert b.spec.psdu_stride % 2 == 1
    assert b.meant[b.recs["psdu_len"] == b.spec.psdu_stride].all() and not b.meant[b.recs["psdu_len"] == b.spec.psdu_stride + 1].any()


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", sr.SHAPE_SPECS)
def test_shapes(capi, name, fmt):
    """1 / 63 / 64 / 65 / 129 / 1040 frames; undecodable records in every lane's first slots and first of every rate; one
    rate (no permutation); only the second rate of every class"""
    check(capi, name, fmt)


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("name", sr.LLR_BITS_SPECS)
def test_narrow_llr_rows(capi, name, fmt):
    """llr_bits 1, 2, 4, 6: the row stride follows llr_bits, a frame's symbols are packed by its own n_bpsc, frames of
    wider rates come back untouched"""
    check(capi, name, fmt)


# ---- few waves, many tasks ----

def task_budget(b, n_waves):
    n_tasks, longest = sr.n_tasks_and_longest(b)
    assert n_tasks >= 12 and n_tasks >= 4 * n_waves
    return n_waves * sr.soft_slice(longest) + 64          # room for n_waves slices, not for one more


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("n_waves", [1, 2, 3])
@pytest.mark.parametrize("name", sr.TASK_SPECS)
def test_few_waves_many_tasks(capi, monkeypatch, name, n_waves, fmt):
    """a scratch budget of one, two and three waves for sixteen tasks (two per rate, four per class): every wave takes
    several tasks, of both rates of its class -- fresh metrics, the previous task's rows, survivor slice and decoded words
    behind it.  The reference knows nothing of waves, so the result is also that of the unconstrained run."""
    sr.check_conditions(name, fmt)
    b, fr, psdu, _ = sr.reference(name, fmt)
    monkeypatch.setenv("WIFIRX_TEST_DECODE_BUDGET", str(task_budget(b, n_waves)))
    ps, res = run_batch(capi, b)
    assert_equals_reference(b, fr, psdu, ps, res[0])


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("fails", [1, 2])
def test_scratch_allocation_falls_back_to_fewer_waves(capi, monkeypatch, fails, fmt):
    """the first allocations of the survivor scratch fail: half the waves, and again (16 -> 8 -> 4), the same bytes"""
    b, fr, psdu, _ = sr.reference("tasks_noisy", fmt)
    assert sr.n_tasks_and_longest(b)[0] == 16
    monkeypatch.setenv("WIFIRX_TEST_FAIL_DECODE_SCRATCH", str(fails))
    ps, res = run_batch(capi, b)
    assert_equals_reference(b, fr, psdu, ps, res[0])


@pytest.mark.parametrize("fmt", sr.FORMATS)
def test_scratch_exhausted_is_enomem_and_recovers(capi, monkeypatch, fmt):
    """four failing allocations: the first call halves 16 -> 8 -> 4 waves, uses three of them up and returns WIFIRX_ENOMEM
    with records and PSDU buffer untouched; the second call on the same handle meets the last one, halves once, and decodes"""
    b, fr, psdu, _ = sr.reference("tasks_nonfinite", fmt)
    assert sr.n_tasks_and_longest(b)[0] == 16
    monkeypatch.setenv("WIFIRX_TEST_FAIL_DECODE_SCRATCH", "4")
    ps, res = run_batch(capi, b, calls=3)
    rc, frames, raw = res[0]
    assert rc == capi.ENOMEM
    assert np.array_equal(frames, b.recs) and (raw == sr.FILL).all()
    assert_equals_reference(b, fr, psdu, ps, res[1])
    assert_equals_reference(b, fr, psdu, ps, res[2])


# ---- hostile samples through the whole soft chain ----

def fuzz_cases():
    """test_gpu_fuzz.CASES, and the frames of its `frames_huge` at further scales.  `frames_huge` itself (x 1e12) is beyond
    what the detector accepts (it finds nothing above about 2e8, where |x|^4 leaves float32), so "scaled further" can
    only mean towards the edges from inside: x 1e8 is the largest scale that still gives frames -- channel-state-weighted
    LLRs of 7e19, the largest a demodulation can emit for these frames --, x 1e-12 the smallest (7e-21).  Weighted
    LLRs outside float32's finite range cannot be had through the demodulator; the host-made `huge` rows cover them."""
    import test_gpu_fuzz
    cases = dict(test_gpu_fuzz.CASES)
    for extra in (1e-24, 1e-12, 1e-8, 1e-4):
        cases["frames_huge_x%.0e" % extra] = (cases["frames_huge"] * np.float32(extra)).astype(np.complex64)
    return cases


FUZZ_NAMES = sorted(fuzz_cases())


@pytest.mark.parametrize("fmt", sr.FORMATS)
@pytest.mark.parametrize("csi", [0, 1])
def test_hostile_samples_through_demod_and_soft_decode(capi, csi, fmt):
    """test_gpu_fuzz's inputs and its frames at four more scales through wifirx_demod_batch (llr_bits 6) and wifirx_decode_batch_soft:
    the reference decodes the rows the DEVICE wrote (downloaded before the decode), so whatever the demodulation emits
    -- NaN, inf, subnormals, 1e38 -- the decoder must treat as rule 14 says.  All frames of all cases are compared."""
    cases = fuzz_cases()
    seen = dict(decoded=0, crc_ok=0, nonfinite_in_decoded=0, all_nan=0, llr_max=0.0, llr_min=np.inf)
    rx = capi.WifiRx(max_sym=40, llr_bits=6, device=0, llr_format=fmt)
    try:
        rx.set_param(capi.P_LLR_CSI, csi)
        for name in FUZZ_NAMES:
            x = np.ascontiguousarray(cases[name])
            n, L = x.shape
            dev = rx.alloc_out(n)
            d_iq = rx.alloc(x.nbytes).upload(x.reshape(-1))
            ps = Fenced(rx, n, 512, 0)
            try:
                rx.demod_batch_dev(d_iq.ptr, L, n, dev)
                rx.sync()
                r0 = rx.download_out(dev, n)
                rc, frames, raw = soft_decode(capi, rx, dev["frames"], dev["llr"], ps, n)
            finally:
                d_iq.free()
                rx.free_out(dev)
                ps.free()
            rows = bf16_to_f32(r0["llr"]) if fmt == "bf16" else r0["llr"]
            nan = np.zeros(n, bool)
            fr, psdu = ref.decode_batch(r0["frames"], rows, 40, psdu_stride=512, nan_out=nan)
            assert rc == 0, name
            assert np.array_equal(frames, fr), name
            want = np.full((n, 512), sr.FILL, np.uint8)
            dec = np.nonzero((fr["flags"] & ref.F_DECODED) != 0)[0]
            for k in dec:
                want[k, :fr["psdu_len"][k]] = psdu[k, :fr["psdu_len"][k]]
                v = np.abs(rows[k, :int(sr.extent(fr)[k])])
                seen["nonfinite_in_decoded"] += int((~np.isfinite(v)).sum())
                seen["llr_max"] = max(seen["llr_max"], float(v[np.isfinite(v)].max()))
                seen["llr_min"] = min(seen["llr_min"], float(v[v > 0].min()))
            assert np.array_equal(raw, ps.expected(want)), name
            seen["decoded"] += dec.size
            seen["crc_ok"] += int(((fr["flags"] & ref.F_CRC_OK) != 0).sum())
            seen["all_nan"] += int(nan.sum())
    finally:
        rx.close()
    print(csi, fmt, seen)
    assert seen["decoded"] >= 6 * 32 and seen["crc_ok"] >= 4 * 32
    if csi:
        assert seen["llr_max"] > 1e19 and seen["llr_min"] < 1e-22          # the edges of what the demodulation emits
