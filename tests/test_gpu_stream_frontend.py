"""Stream mode with the front end on (wifirx_stream_frontend, NUMERICS.md rule 32): scenes (a) and (b) of
tests/frontend_scene.py through push / push_iq.  The frames are those of the oracle's stream receiver on the restated front
end's output, whatever the chunking, and the state read back is the restatement's."""
import numpy as np
import pytest

import frontend_ref as fr
import frontend_scene as sc

pytestmark = pytest.mark.gpu

MAX_SYM = 64
# per scene: the front end's flags, and the integer format the scene is also pushed in: (format, quantiser scale, widening scale)
ARMS = {"a": (fr.FE_DC, (fr.SC8, 1.0, 1.0)), "b": (fr.FE_DC | fr.FE_IQ, (fr.SC16, 256.0, 2.0 ** -8))}


@pytest.fixture(scope="module")
def scenes(orc):
    """per (scene, format): the samples to push, the widening scale, the restated output's oracle frames and PSDU rows, the
    restated state, the late slots that must decode"""
    out = {}
    for name, (flags, (ifmt, qscale, wscale)) in ARMS.items():
        x, psdus, slot_len = sc.build(name)
        q = np.clip(np.rint(fr.widen(x) * np.float32(qscale)), -32768 if ifmt == fr.SC16 else -128, 32767 if ifmt == fr.SC16 else 127)
        q = q.astype(np.int16 if ifmt == fr.SC16 else np.int8)
        for fmt, data, scale in ((fr.FC32, x, 1.0), (ifmt, q, wscale)):
            z, st = fr.frontend(data, fmt, scale, flags=flags)
            good, o, rows = sc.oracle_good(orc, z, psdus, slot_len, max_sym=MAX_SYM)
            late = set(sc.late_slots(slot_len))
            assert good & late == late                      # the scene's condition holds for what is pushed
            raw = fr.widen(data, fmt, scale).view(np.complex64).reshape(-1)
            out[name, fmt] = dict(data=data, scale=scale, flags=flags, frames=o["frames"], psdu=rows, state=st, raw=raw,
                                  raw_oracle=sc.oracle_good(orc, raw, psdus, slot_len, max_sym=MAX_SYM)[1:])
    return out


def cfg_of(flags):
    from wifirx import capi
    return capi.frontend_cfg(dc=bool(flags & fr.FE_DC), iq=bool(flags & fr.FE_IQ))


def push_all(rx, s, fmt, cuts):
    """the scene in pieces cut at `cuts`, then a flush; returns (frames, psdu rows)"""
    data = s["data"]
    n = len(data)
    got = []
    for a, b in zip([0] + list(cuts), list(cuts) + [n]):
        if fmt == fr.FC32:
            rx.push(data[a:b])
        else:
            rx.push_iq(data[a:b], scale=s["scale"])
        got.append(rx.poll(cap=256))
    rx.flush()
    got.append(rx.poll(cap=256))
    return np.concatenate([g["frames"] for g in got]), np.concatenate([g["psdu"] for g in got])


def cuts_of(n, chunking):
    if chunking == "whole":
        return []
    if chunking == "random":
        rng = np.random.default_rng(5)
        return [int(c) for c in np.cumsum(rng.integers(1, 9001, size=64)) if c < n]          # (64 pieces cover every scene)
    return list(range(chunking, n, chunking))


def check(frames, psdu, s):
    from wifirx import capi
    assert len(frames) == len(s["frames"])
    assert np.array_equal(frames, s["frames"]), (frames, s["frames"])
    for k in range(len(frames)):
        if frames[k]["flags"] & capi.F_CRC_OK:
            L = int(frames[k]["psdu_len"])
            assert np.array_equal(psdu[k, :L], s["psdu"][k, :L])


@pytest.mark.parametrize("chunking", ["whole", 8192, 1000, "random"])
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("name", ["a", "b"])
def test_scene_through_the_stream(scenes, name, integer, chunking):
    from wifirx import capi
    fmt = ARMS[name][1][0] if integer else fr.FC32
    s = scenes[name, fmt]
    rx = capi.WifiRx(max_sym=MAX_SYM)
    try:
        rx.stream_frontend(cfg_of(s["flags"]))
        frames, psdu = push_all(rx, s, fmt, cuts_of(len(s["data"]), chunking))
        check(frames, psdu, s)
        assert rx.stream_frontend_state().tobytes() == s["state"].tobytes()
    finally:
        rx.close()


@pytest.mark.parametrize("integer", [False, True])
def test_scene_through_the_worker_thread(scenes, integer):
    """host input with a batch size: the pushes are staged and the pipeline, the front end included, runs on the worker"""
    from wifirx import capi
    fmt = ARMS["b"][1][0] if integer else fr.FC32
    s = scenes["b", fmt]
    rx = capi.WifiRx(max_sym=MAX_SYM)
    try:
        rx.set_param(capi.P_STREAM_BATCH, 20000)
        rx.stream_frontend(cfg_of(s["flags"]))
        frames, psdu = push_all(rx, s, fmt, cuts_of(len(s["data"]), 1000))
        check(frames, psdu, s)
        assert rx.stream_frontend_state().tobytes() == s["state"].tobytes()
    finally:
        rx.close()


def test_initial_state_and_device_input(scenes):
    """a stream that starts from a given state (the second half of scene (b) from the state behind the first half), pushed
    from device memory"""
    from wifirx import capi
    s = scenes["b", fr.SC16]
    half = 5 * 4096 + 123
    fe = fr.Frontend(flags=s["flags"])
    fe.process(s["data"][:half], fr.SC16, s["scale"])
    init = fe.state()
    z = fe.process(s["data"][half:], fr.SC16, s["scale"])
    rx, ref = capi.WifiRx(max_sym=MAX_SYM), capi.WifiRx(max_sym=MAX_SYM)
    tail = np.ascontiguousarray(s["data"][half:])
    d = rx.alloc(tail.nbytes).upload(tail)
    try:
        rx.stream_frontend(cfg_of(s["flags"]), init)
        rx.push_iq_dev(d.ptr, len(tail), fr.SC16, s["scale"])
        rx.flush()
        got = rx.poll(cap=256)
        ref.push(z)                                          # the restated output through a handle without a front end
        ref.flush()
        want = ref.poll(cap=256)
        assert len(got["frames"]) >= 10 and np.array_equal(got["frames"], want["frames"]) and np.array_equal(got["psdu"], want["psdu"])
        assert rx.stream_frontend_state().tobytes() == fe.state().tobytes()
    finally:
        d.free()
        rx.close()
        ref.close()


@pytest.mark.parametrize("fmt", [fr.FC32, fr.SC8])
def test_a_handle_with_the_front_end_off_is_what_it_was(scenes, fmt):
    """never switched on, and switched on and off again before the first sample: the oracle's frames on the raw samples"""
    from wifirx import capi
    s = scenes["a", fmt]
    o, rows = s["raw_oracle"]
    want = dict(frames=o["frames"], psdu=rows)
    for toggle in (False, True):
        rx = capi.WifiRx(max_sym=MAX_SYM)
        try:
            if toggle:
                rx.stream_frontend(cfg_of(3))
                rx.stream_frontend(None)
                with pytest.raises(capi.WifiRxError) as e:
                    rx.stream_frontend_state()
                assert e.value.code == capi.EINVAL
            frames, psdu = push_all(rx, s, fmt, cuts_of(len(s["data"]), 8192))
            check(frames, psdu, want)
        finally:
            rx.close()


def test_a_failed_push_leaves_the_state_unchanged(scenes, monkeypatch):
    """the injected allocation failures of tests/test_gpu_stream.py with the front end on: the push that fails has consumed
    nothing, the state is what it was in front of it, and the stream pushed again gives the undisturbed frames and state"""
    from wifirx import capi
    s = scenes["a", fr.FC32]
    x = s["data"]
    chunk = 10000
    failures = 0
    for k in range(1, 12):
        monkeypatch.setenv("WIFIRX_TEST_FAIL_ALLOC", str(k))
        rx = capi.WifiRx(max_sym=MAX_SYM)
        try:
            rx.stream_frontend(cfg_of(s["flags"]))
            got = []
            for p in range(0, x.size, chunk):
                before = rx.stream_frontend_state()
                try:
                    rx.push(x[p:p + chunk])
                except capi.WifiRxError as e:
                    assert e.code == capi.ENOMEM, str(e)
                    failures += 1
                    assert rx.push_consumed() == 0
                    assert rx.stream_frontend_state().tobytes() == before.tobytes(), k
                    rx.push(x[p:p + chunk])
                assert int(rx.stream_frontend_state()["n"]) == min(p + chunk, x.size)
                got.append(rx.poll(cap=256))
            rx.flush()
            got.append(rx.poll(cap=256))
            check(np.concatenate([g["frames"] for g in got]), np.concatenate([g["psdu"] for g in got]), s)
            assert rx.stream_frontend_state().tobytes() == s["state"].tobytes(), k
        finally:
            rx.close()
    assert failures >= 6                # some of them behind the front end's launches: the output buffers of the first frames


def test_diversity_refuses(scenes):
    from wifirx import capi
    x = scenes["a", fr.FC32]["data"][:20000]
    rx = capi.WifiRx(max_sym=MAX_SYM)
    try:
        rx.stream_frontend(cfg_of(1))
        with pytest.raises(capi.WifiRxError) as e:
            rx.push_diversity([x, x])
        assert e.value.code == capi.EINVAL and "front end" in str(e.value)
    finally:
        rx.close()
    rx = capi.WifiRx(max_sym=MAX_SYM)
    try:
        rx.push_diversity([x, x])
        with pytest.raises(capi.WifiRxError) as e:
            rx.stream_frontend(cfg_of(1))
        assert e.value.code == capi.EINVAL
        rx.stream_frontend(None)                             # switching off is always possible
    finally:
        rx.close()


def test_switch_argument_checks():
    from wifirx import capi
    rx = capi.WifiRx(max_sym=MAX_SYM)
    try:
        for bad in (capi.FrontendCfg(4, 12, 2, 4), capi.FrontendCfg(1, 31, 2, 4), capi.FrontendCfg(1, 12, 7, 4), capi.FrontendCfg(1, 12, 2, 7)):
            with pytest.raises(capi.WifiRxError) as e:
                rx.stream_frontend(bad)
            assert e.value.code == capi.EINVAL
        assert capi.lib().wifirx_stream_frontend(None, None, None) == capi.EINVAL
        assert capi.lib().wifirx_stream_frontend_state(rx._h, None) == capi.EINVAL
    finally:
        rx.close()
