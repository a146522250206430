"""wifirx_decode_batch on the MI355X, byte for byte, on records and hard decisions made on the host (tests/hard_rows.py) -- no
demodulator in the loop, so the decoders meet what no transmission gives them: uniformly random decisions (two frames in
three end with several states at the minimum, nearly every frame passes ties on its surviving path, the speculative
walks of decode_q_kernel break), all-0 and all-0xFF rows, garbage above the rate's bits, next to real frames with and
without bit flips.  Five decoder paths: the wave-per-frame kernel, decode_kernel with partly and with fully filled
waves, decode_q_kernel with the trace-back behind each task and with the speculative one.

Every comparison is over whole arrays: all frame records, every byte of a PSDU allocation that was filled with 0xA5 and
sits between fences (bytes 0 .. psdu_len - 1 of the decoded frames equal the reference, everything else still holds the
pattern), and the decisions, which must come back unchanged.  The reference is the oracle's decode_mac, once per batch;
tests/test_hard_rows.py shows on the CPU that it equals the independent tests/hard_viterbi_ref.py on every batch of the
table and that the batches are what they claim to be.

Wall time of the module on an MI355X: 7 s for its 244 tests (the slowest 0.3 s).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import hard_rows as hr
from helpers import Fenced

pytestmark = pytest.mark.gpu

PATHS = {
    "small":     {"WIFIRX_DECODE_SMALL_MAX": "1000000000"},
    "pair":      {"WIFIRX_DECODE_SMALL_MAX": "0", "WIFIRX_DECODE_Q": "0"},
    "pair_full": {"WIFIRX_DECODE_SMALL_MAX": "0", "WIFIRX_DECODE_Q": "0", "WIFIRX_DECODE_FPW": "128"},
    "q0":        {"WIFIRX_DECODE_SMALL_MAX": "0", "WIFIRX_DECODE_Q": "1", "WIFIRX_DECODE_FPW": "256", "WIFIRX_DECODE_OVL": "0"},
    "q2":        {"WIFIRX_DECODE_SMALL_MAX": "0", "WIFIRX_DECODE_Q": "1", "WIFIRX_DECODE_FPW": "256", "WIFIRX_DECODE_OVL": "2"},
}
ALL_PATHS = tuple(PATHS)
Q_BUDGET = 3_000_000          # WIFIRX_TEST_DECODE_BUDGET of test_gpu_parity.test_decode_mac_scratch_fallbacks


@pytest.fixture(scope="module")
def capi():
    from wifirx import capi
    return capi


@pytest.fixture
def path(request, monkeypatch):
    """the decoder path of the handles this test creates: the library reads these when a handle is created"""
    for k in ("WIFIRX_DECODE_SMALL_MAX", "WIFIRX_DECODE_Q", "WIFIRX_DECODE_FPW", "WIFIRX_DECODE_OVL", "WIFIRX_TEST_DECODE_BUDGET",
              "WIFIRX_TEST_FAIL_DECODE_SCRATCH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def on_paths(*names):
    return pytest.mark.parametrize("path", names, indirect=True)


class Decisions:
    """the decisions of a batch on the device, `off` bytes behind a 16-byte boundary: `idx` [n][max_sym][48], or their bit
    planes [n][max_sym * 12] (the form decode_mac reads; then there is no `idx` buffer at all)"""

    def __init__(self, rx, b, max_sym, planes=False, off=0):
        assert not (planes and off)
        host = b.planes() if planes else b.idx
        if max_sym != b.spec.max_sym:          # a handle with longer rows: the batch's rows at the handle's stride
            assert not planes and max_sym > b.spec.max_sym
            wide = np.zeros((b.recs.size, max_sym, 48), np.uint8)
            wide[:, :b.spec.max_sym] = host
            host = wide
        self.host = np.concatenate([np.full(off, 0x5A, np.uint8), np.ascontiguousarray(host).view(np.uint8).reshape(-1),
                                    np.full(16 - off, 0x5A, np.uint8)])
        self.buf = rx.alloc(self.host.nbytes).upload(self.host)
        assert self.buf.ptr % 16 == 0
        self.idx = None if planes else self.buf.ptr + off
        self.hbits = self.buf.ptr if planes else None

    def unchanged(self):
        return np.array_equal(self.buf.download(np.uint8, self.host.size), self.host)

    def free(self):
        self.buf.free()


def decode(capi, rx, d_frames, dec, ps, n):
    """wifirx_decode_batch over device buffers; returns (rc, records, the whole PSDU allocation)"""
    out = capi.Out(d_frames.ptr, dec.idx, None, None, ps.ptr, ps.stride, 1, None, None, dec.hbits)
    rc = capi.lib().wifirx_decode_batch(rx._h, n, C.byref(out))
    rx.sync()
    return rc, d_frames.download(capi.FRAME_DTYPE, n), ps.download()


@functools.lru_cache(maxsize=None)
def expected(name, stride=None):
    """(batch, the oracle's records, the PSDU rows a 0xA5-filled buffer of that stride must hold afterwards); once per batch"""
    b, fr, psdu = hr.oracle_reference(name)
    assert stride is None or (b.recs["psdu_len"] <= min(stride, b.spec.psdu_stride)).all()      # the stride decides nothing here
    rows = hr.expected_psdu_buffer(b, fr, psdu, stride)
    rows.setflags(write=False)
    return b, fr, rows


def assert_equals_reference(fr, rows, ps, dec, got):
    rc, frames, raw = got
    assert rc == 0
    assert np.array_equal(frames, fr), np.nonzero(frames != fr)[0][:8]
    want = ps.expected(rows)
    assert np.array_equal(raw, want), np.nonzero(raw != want)[0][:8] - ps.at
    assert dec.unchanged()


def check(capi, name, planes=False, psdu_off=0, idx_off=0, stride=None):
    """the batch through a handle of its own"""
    b, fr, rows = expected(name, stride)
    n = b.recs.size
    rx = capi.WifiRx(max_sym=b.spec.max_sym, llr_bits=0, device=0)
    try:
        d_fr = rx.alloc(n * 32).upload(b.recs)
        dec = Decisions(rx, b, b.spec.max_sym, planes, idx_off)
        ps = Fenced(rx, n, rows.shape[1], psdu_off)
        try:
            assert_equals_reference(fr, rows, ps, dec, decode(capi, rx, d_fr, dec, ps, n))
        finally:
            for d in (d_fr, dec, ps):
                d.free()
    finally:
        rx.close()
    return b, fr


@on_paths(*ALL_PATHS)
@pytest.mark.parametrize("name", hr.VALUE_SPECS)
def test_values(capi, path, name):
    """every decision class x all eight rates in one batch (grouped by rate on the device), 264 frames per rate in three
    lengths: a full and a ragged 256-frame task per rate, the 64-QAM instance of decode_q_kernel"""
    b, fr = check(capi, name)
    assert b.recs.size == 2112 and b.meant.all()


@on_paths("pair_full", "q0", "q2")
@pytest.mark.parametrize("name", ("values_random", "values_flips"))
def test_values_from_planes_only(capi, path, name):
    """the same decisions as bit planes, out.idx = NULL: no pack pre-pass, the caller's planes are what the kernels read"""
    check(capi, name, planes=True)


@on_paths(*ALL_PATHS)
def test_ladder(capi, path):
    """1 .. 10 symbols at every rate, psdu_len 0 .. 3, random decisions: trellises of 24 .. 2160 steps share their tasks
    (lanes ending while their wave goes on; decode_q_kernel's mode 2 walks such tasks back on the spot)"""
    check(capi, "ladder")


@on_paths(*ALL_PATHS)
@pytest.mark.parametrize("name", hr.UNIFORM_SPECS)
def test_uniform(capi, path, name):
    """300 frames of one rate and length, random decisions: the speculative trace-back proper, with walks that break; trellises
    that end on a block boundary of 96 steps, just behind one and just before the next (hard_rows.UNIFORM_REMAINDERS)"""
    check(capi, name)


@on_paths(*ALL_PATHS)
@pytest.mark.parametrize("name", hr.LONG_SPECS)
def test_longest_frames(capi, path, name):
    """1528 bytes on a max_sym = 511 handle (12 264 .. 12 384 steps: the largest scratch slice, the longest chain of walks, over a
    hundred normalisations of the 16-bit metrics and 255 of the bytes); 1529 bytes left alone"""
    b, fr = check(capi, name)
    assert (b.recs["psdu_len"] == hr.MAX_PSDU + 1).sum() == 1 and b.meant.sum() == 64


@on_paths("small", "pair_full", "q2")
@pytest.mark.parametrize("name", hr.EDGE_SPECS)
def test_edges(capi, path, name):
    """n_sym == max_sym decoded, max_sym + 1 left alone; psdu_len == psdu_stride (odd) decoded, psdu_stride + 1 left alone;
    psdu_len 0 .. 8; records that are not decodable in the first 64 slots (no COMPLETE, PSDU longer than the row)"""
    check(capi, name)


@on_paths("pair_full", "q2")
@pytest.mark.parametrize("name", hr.N_SPECS)
def test_shapes(capi, path, name):
    """1 .. 513 frames around the 64 lanes, the 128 and the 256 frames of a task"""
    check(capi, name)


@on_paths("small", "pair_full", "q2")
@pytest.mark.parametrize("off", [1, 2, 3])
def test_unaligned_buffers(capi, path, off):
    """the PSDU buffer 1 .. 3 bytes behind a 16-byte boundary with an odd stride (finish_frame stores byte by byte), the `idx`
    pointer one byte behind a boundary (the pack pre-pass assembles its words from bytes)"""
    check(capi, "values_flips", psdu_off=off, idx_off=1, stride=97)


@on_paths("pair_full", "q0", "q2")
def test_one_handle_several_calls(capi, path):
    """long_0_random, values_random, n_1 on ONE max_sym = 511 handle, each equal to its own reference: nothing of the larger
    earlier call -- survivor scratch, the pre-pass counters and cursors, the 0xff-filled permutation, the handle-owned planes
    -- leaks into the later ones.  Then values_flips, and wifirx_decode_batch once more in place on its finished records
    (DECODED and CRC_OK set): records and bytes stay as they are."""
    rx = capi.WifiRx(max_sym=511, llr_bits=0, device=0)
    try:
        for name in ("long_0_random", "values_random", "n_1", "values_flips"):
            b, fr, rows = expected(name)
            assert b.meant.all() or name.startswith("long")          # no frame is held back by the batch's own max_sym
            n = b.recs.size
            d_fr = rx.alloc(n * 32).upload(b.recs)
            dec = Decisions(rx, b, 511)
            ps = Fenced(rx, n, rows.shape[1])
            try:
                assert_equals_reference(fr, rows, ps, dec, decode(capi, rx, d_fr, dec, ps, n))
                if name == "values_flips":
                    assert_equals_reference(fr, rows, ps, dec, decode(capi, rx, d_fr, dec, ps, n))
            finally:
                for d in (d_fr, dec, ps):
                    d.free()
    finally:
        rx.close()


def q_slice(n_steps, spec):
    """dec_q_slice of csrc/wr_kernels.h: the scratch bytes of one wave of decode_q_kernel"""
    return n_steps * 64 * 32 + (n_steps // 32 + 2) * 256 * 4 + ((n_steps // 96 + 2) * 64 * 4 if spec else 0)


@on_paths("q0", "q2")
def test_fewer_waves_than_tasks(capi, path, monkeypatch):
    """a scratch budget of two waves for the sixteen tasks of values_random: every wave takes eight tasks in turn, of several
    rates, with broken links in each"""
    b = hr.build("values_random")
    steps = int((b.recs["n_sym"].astype(np.int64) * np.array(hr.N_DBPS)[b.recs["encoding"]]).max())
    n_tasks = sum(-(-int((b.recs["encoding"] == e).sum()) // 256) for e in range(8))
    assert n_tasks == 16 and 1 <= Q_BUDGET // q_slice(steps, path == "q2") < n_tasks // 4
    monkeypatch.setenv("WIFIRX_TEST_DECODE_BUDGET", str(Q_BUDGET))
    check(capi, "values_random")
