"""Time wifirx_mac_batch and wifirx_link_stats at config 3's geometry (one million 294-byte PSDUs, 11 data symbols of 64-QAM)
with HIP events on the handle's stream after a warm-up, alternating in one process with device-to-device hipMemcpyAsync calls
that move as many bytes as each kernel reads + writes.  A timed window holds enough repetitions to last about 0.1 s or more;
the figures are per call, medians over the windows.  The batch that is scored is a clean loop-back (TX rows demodulated and
decoded without a channel): every frame is good and CRC_OK, so link_stats reads every record, PSDU and decision row -- its
largest byte count.  wifirx_link_stats waits for its 72 bytes, so its figure is the whole call (memset, kernel, copy, wait).
Prints one JSON line, writes it to --out when given.

    python tools/link_bench.py [--frames 1000000] [--windows 5] [--out profiles/link_config3.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnuradio-wifi-imagetransfer_amd")]

from wifirx import capi, txgen  # noqa: E402

SLOT, LEAD, ENC, PSDU_LEN = 1472, 160, 7, 294
AIM = 1.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_000_000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames
    n_sym, nb = txgen.n_sym_for(PSDU_LEN, ENC), txgen.RATE_TABLE[ENC][0]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    rx = capi.WifiRx(max_sym=n_sym, chan_est=capi.EQ_LS, device=0)
    st = C.c_void_p(rx.stream_ptr())
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0

    pay_len = PSDU_LEN - 28
    d_pay = rx.alloc(n * pay_len)
    d_psdu = rx.alloc(n * PSDU_LEN)
    rows = rx.alloc(n * SLOT * 8)
    rx.mac_batch_dev(d_pay.ptr, pay_len, n, None, payload_len=pay_len - 28, payload_seed=5)      # some bytes to frame
    rx.mac_batch_dev(d_psdu.ptr, PSDU_LEN, n, None, payload_len=pay_len, payload_seed=1)
    rx.tx_batch_dev(rows.ptr, n * SLOT, d_psdu.ptr, ENC, psdu_len=np.full(n, PSDU_LEN, np.uint32), psdu_stride=PSDU_LEN,
                    lead=LEAD, row_len=SLOT)
    dev = rx.alloc_out(n, psdu_stride=304, want_hbits=True)
    ref = rx.alloc_out(n, want_hbits=True)
    ref["psdu"], ref["psdu_stride"] = d_psdu, PSDU_LEN
    rx.demod_batch_dev(rows.ptr, SLOT, n, ref)
    rx.demod_batch_dev(rows.ptr, SLOT, n, dev)
    rx.decode_batch_dev(n, dev)
    full = rx.link_stats(n, dev, ref)
    assert full["frames_good"] == full["frames_psdu_ok"] == n and full["coded_bit_errors"] == 0, full
    rows.free()
    d_err, d_cls, d_mac = rx.alloc(4 * n), rx.alloc(n), rx.alloc(n * PSDU_LEN)
    only = lambda d, *keys: {k: v for k, v in d.items() if k in keys or k in ("frames", "psdu", "psdu_stride")}
    cnt = capi.LinkCounts()
    lib = capi.lib()

    def stats_call(d_rx, d_ref, per_frame):
        o_rx, o_ref = rx._out_struct(d_rx), rx._out_struct(d_ref)
        pe, pc = (d_err.ptr, d_cls.ptr) if per_frame else (None, None)
        return lambda: lib.wifirx_link_stats(rx._h, n, C.byref(o_rx), C.byref(o_ref), pe, pc, C.byref(cnt))

    b_rec, b_psdu, b_dec = 2 * 32 * n, 2 * PSDU_LEN * n, 2 * n_sym * 48 * n
    # name -> (call, bytes read + written)
    ops = {
        "mac_philox": (lambda: lib.wifirx_mac_batch(rx._h, None, 0, pay_len, None, n, None, 0, 1, d_mac.ptr, PSDU_LEN), PSDU_LEN * n),
        "mac_device_payload": (lambda: lib.wifirx_mac_batch(rx._h, d_pay.ptr, 1, pay_len, None, n, None, 0, 0, d_mac.ptr, PSDU_LEN),
                               (pay_len + PSDU_LEN) * n),
        "link_stats_idx": (stats_call(only(dev, "idx"), only(ref, "idx"), False), b_rec + b_psdu + b_dec),
        "link_stats_hbits": (stats_call(dev, ref, False), b_rec + b_psdu + b_dec),
        "link_stats_hbits_per_frame": (stats_call(dev, ref, True), b_rec + b_psdu + b_dec + 5 * n),
    }
    scratch = rx.alloc(max(b for _, b in ops.values()) + 512)
    copies = {}
    for name, (_, nbytes) in ops.items():
        half = nbytes // 2
        copies.setdefault(nbytes, lambda half=half: hip.hipMemcpyAsync(scratch.ptr + ((half + 255) & ~255), scratch.ptr, half, 3, st))

    def window(fn, reps):
        assert hip.hipEventRecord(ev0, st) == 0
        for _ in range(reps):
            assert fn() == 0
        assert hip.hipEventRecord(ev1, st) == 0
        assert hip.hipEventSynchronize(ev1) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), ev0, ev1) == 0
        return t.value / reps

    runs = {name: fn for name, (fn, _) in ops.items()}
    runs.update({"memcpy_%d" % b: fn for b, fn in copies.items()})
    reps = {}
    for name, fn in runs.items():                                        # warm-up, and the repetitions of a 0.1 s window
        window(fn, 3)
        reps[name] = max(int(np.ceil(120.0 / max(window(fn, 10), 1e-3))), 10)
    ms = {k: [] for k in runs}
    for _ in range(a.windows):                                           # alternate them
        for name, fn in runs.items():
            ms[name].append(window(fn, reps[name]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ratio = {name: med[name] / med["memcpy_%d" % b] for name, (_, b) in ops.items()}
    res = dict(workload="config 3's geometry: %d frames, PSDU %d B (payload %d B), %d data symbols of 64-QAM; clean loop-back scored"
                        % (n, PSDU_LEN, pay_len, n_sym),
               bytes_read_plus_written={name: b for name, (_, b) in ops.items()}, reps_per_window=reps, ms_windows=ms,
               mac_ms=med["mac_philox"], mac_device_payload_ms=med["mac_device_payload"],
               link_stats_ms={"idx": med["link_stats_idx"], "hbits": med["link_stats_hbits"],
                              "hbits_per_frame": med["link_stats_hbits_per_frame"]},
               memcpy_d2d_ms={str(b): med["memcpy_%d" % b] for b in copies},
               GBps={name: b / med[name] / 1e6 for name, (_, b) in ops.items()},
               ratio_to_memcpy=ratio, aim_ratio=AIM, meets_aim={name: bool(r <= AIM) for name, r in ratio.items()},
               note="every figure is per call, HIP events around a window of calls; the memcpy of an entry moves half its byte "
                    "count (it reads and writes each byte it moves); wifirx_link_stats waits for its counters, so its figure "
                    "holds the memset, the kernel, the 72-byte copy and the wait of a call")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    for d in (d_pay, d_err, d_cls, d_mac, scratch):
        d.free()
    rx.free_out(dev)
    rx.free_out(ref)
    rx.close()


if __name__ == "__main__":
    main()
