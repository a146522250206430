"""The DEVICE against the float64 restatement of the prose, without the oracle in between: LMS / COMB / STA, points, LLRs,
CSI, moments -- and the device against the oracle byte for byte OFF the default (bandwidth, frequency).

`tests/test_gpu_independent.py` holds the hard decisions of the LS equaliser at 20 MHz / 5.89 GHz against
`tests/independent_rx.py`.  This module runs the cases of `tests/independent_eq_cases.py` (the same inputs, tolerances and
compared-symbol rule as the CPU test `tests/test_independent_eq.py`) through `capi.WifiRx` with all four equalisers at three
operating points: what the kernels compute IS what NUMERICS.md rules 7, 9, 11, 12, 13 say in words, to float32 rounding.
bandwidth / frequency scales the sampling-offset compensation of every symbol (rule 9), and no other test of the device
leaves the default: the byte parity with the oracle's SPEC mode is held at the two other points here, for a handle created
there and for one moved there with `set_param`."""
import numpy as np
import pytest

import independent_eq_cases as C

pytestmark = pytest.mark.gpu

OFF_DEFAULT = [op for op in C.OPS if op != C.DEFAULT_OP]
OP_ID = lambda op: "%gMHz_%gGHz" % (op[0] / 1e6, op[1] / 1e9)
RAW = ("frames", "idx", "llr", "carrier", "csi", "sym_stats")
_device = {}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run(rx, name):
    iq, _ = C.slots_of(name)
    return rx.demod_batch(iq.reshape(-1), iq.shape[1], want_csi=True, want_stats=True)


def handle(name, chan_est, op):
    from wifirx import capi
    _, max_sym = C.slots_of(name)
    return capi.WifiRx(bandwidth=op[0], frequency=op[1], chan_est=chan_est, max_sym=max_sym,
                       llr_bits=C.N_BPSC[C.CASES[name][0]], want_carrier=True)


def device_outputs(name, chan_est, op):
    """one handle created at `op`: a run without and a run with the channel-state weight; once per module"""
    from wifirx import capi
    key = (name, chan_est, op)
    if key not in _device:
        rx = handle(name, chan_est, op)
        try:
            off = run(rx, name)
            rx.set_param(capi.P_LLR_CSI, 1)
            on = run(rx, name)
        finally:
            rx.close()
        _device[key] = dict(off=off, on=on, frames=off["frames"], idx=off["idx"], eq=off["carrier"], llr=off["llr"],
                            llr_csi=on["llr"], csi=off["csi"], sym_stats=off["sym_stats"])
    return _device[key]


@pytest.mark.parametrize("op", C.OPS, ids=OP_ID)
@pytest.mark.parametrize("name", list(C.CASES))
def test_device_agrees_with_the_reference(name, op):
    for ce in range(4):
        out = C.distances(C.reference(name, ce, op), device_outputs(name, ce, op), ce)
        print(name, op, C.EQ_NAMES[ce], out)
        C.check(out, (name, op, C.EQ_NAMES[ce]))


@pytest.mark.parametrize("op", OFF_DEFAULT, ids=OP_ID)
@pytest.mark.parametrize("name", list(C.CASES))
def test_device_equals_the_oracle_off_the_default_operating_point(orc, name, op):
    for ce in range(4):
        d, o = device_outputs(name, ce, op), C.oracle_outputs(orc, name, ce, op)
        for k, ok in (("frames", "frames"), ("idx", "idx"), ("llr", "llr"), ("eq", "eq"), ("csi", "csi"), ("llr_csi", "llr_csi")):
            assert same_bytes(d[k], o[ok]), (name, op, C.EQ_NAMES[ce], k)
        assert same_bytes(d["on"]["frames"], o["frames"]) and same_bytes(d["on"]["idx"], o["idx"])


@pytest.mark.parametrize("chan_est,name", [(0, "long_bpsk"), (1, "qam16"), (2, "qpsk"), (3, "qam64")],
                         ids=["LS-long_bpsk", "LMS-qam16", "COMB-qpsk", "STA-qam64"])
def test_a_handle_moved_with_set_param_equals_one_created_there(chan_est, name):
    from wifirx import capi
    rx = handle(name, chan_est, C.DEFAULT_OP)
    try:
        first = run(rx, name)
        for op in OFF_DEFAULT:
            rx.set_param(capi.P_BANDWIDTH, op[0])
            rx.set_param(capi.P_FREQUENCY, op[1])
            moved = run(rx, name)
            there = device_outputs(name, chan_est, op)["off"]
            for k in RAW:
                assert same_bytes(moved[k], there[k]), (op, k)
            assert not same_bytes(moved["carrier"], first["carrier"]), op          # the operating point does reach the points
            rx.set_param(capi.P_BANDWIDTH, C.DEFAULT_OP[0])
            rx.set_param(capi.P_FREQUENCY, C.DEFAULT_OP[1])
            back = run(rx, name)
            for k in RAW:
                assert same_bytes(back[k], first[k]), (op, k)
    finally:
        rx.close()
    at_default = device_outputs(name, chan_est, C.DEFAULT_OP)["off"]
    for k in RAW:
        assert same_bytes(first[k], at_default[k]), k


@pytest.mark.parametrize("name", list(C.CASES))
def test_channel_state_weight_on_and_off(name):
    """rule 12: with llr_csi on the LLRs are the reference's weighted ones and no decision moves; off again, the bytes return"""
    from wifirx import capi
    op = C.DEFAULT_OP
    for ce in range(4):
        d = device_outputs(name, ce, op)
        ref = C.reference(name, ce, op)
        assert same_bytes(d["on"]["idx"], d["off"]["idx"]) and same_bytes(d["on"]["carrier"], d["off"]["carrier"])
        assert same_bytes(d["on"]["frames"], d["off"]["frames"]) and same_bytes(d["on"]["csi"], d["off"]["csi"])
        out = C.distances(ref, d, ce)
        assert out["llr_csi_rel"] <= C.TOL_LLR_CSI and out["llr"] <= C.TOL_Y, (name, C.EQ_NAMES[ce], out)
        sym, _, _ = C.compared(ref, ce, C.DELTA)
        shape = ref["llr"].shape
        on, off = d["on"]["llr"].reshape(shape)[sym], d["off"]["llr"].reshape(shape)[sym]
        assert np.array_equal(np.signbit(on), np.signbit(off))                     # the weight is positive
        assert (np.abs(on) > np.abs(off)).mean() > 0.9                             # |H|^2 is a few hundred at txgen's scaling
    rx = handle(name, 0, op)
    try:
        rx.set_param(capi.P_LLR_CSI, 1)
        on = run(rx, name)
        rx.set_param(capi.P_LLR_CSI, 0)
        off = run(rx, name)
    finally:
        rx.close()
    d = device_outputs(name, 0, op)                                                 # there the weight went off -> on, here on -> off
    assert same_bytes(on["llr"], d["on"]["llr"]) and same_bytes(off["llr"], d["off"]["llr"])
