"""wifirx_irs_sweep in the C ABI and the Python surface: the declaration, the ctypes prototype and the constructor checks on a
box without a GPU; the host checks of the entry point, which need a handle, on the device."""
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm


def test_symbol_declared_exported_and_listed():
    from wifirx import capi
    assert re.search(r"\bint\s+wifirx_irs_sweep\s*\(", _header())
    assert "wifirx_irs_sweep" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_irs_sweep")
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4          # additive: the version stays


def test_20_arguments_word_for_word():
    import ctypes as C
    from wifirx import capi
    want = ["wifirx_handle* h", "float* taps_out", "uint32_t n_sets", "uint32_t n_taps", "const float* pdp", "float gain",
            "uint32_t n_elems", "const float* los_b2r", "const float* los_r2u", "const float* los_b2u", "float k_factor",
            "float direct_gain", "const float* codebook", "int codebook_on_device", "uint32_t n_codes",
            "const float* scatter", "uint32_t n_scatter", "uint64_t irs_seed", "uint16_t* best_out", "float* power_out"]
    assert _norm(_decl(_header(), "wifirx_irs_sweep")) == want
    kinds = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    types = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in want]
    assert list(capi.lib().wifirx_irs_sweep.argtypes) == types


def test_header_comment_carries_the_rule():
    raw = _header_raw()
    at = raw.index("int  wifirx_irs_sweep(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for word in ("NUMERICS.md rule 26", "(n, r, l, 2)", "0xFFFFFFFF", "(r L + l) % n_scatter", "one fma chain", "from +0",
                 "multiple of 4", "v_mfma_f32_16x16x4_f32", "without fma", "ascending l", "strict >", "lowest k wins a", "NaN power never wins",
                 "all powers NaN give 0", "1 <= n_codes <= 1024", "all three outputs NULL", "ORDER: as wifirx_channel", "WIFIRX_EINVAL"):
        assert word in comment, word


def test_python_surface():
    from wifirx import block, capi, irs
    prm = inspect.signature(capi.WifiRx.irs_sweep_dev).parameters
    assert prm["k_factor"].default == 0.0 and prm["direct_gain"].default == 1.0 and prm["gain"].default == 1.0
    assert prm["scatter"].default is None and prm["seed"].default == 0
    assert prm["codebook"].kind is inspect.Parameter.KEYWORD_ONLY and prm["codebook"].default is inspect.Parameter.empty
    assert prm["best_ptr"].default is None and prm["power_ptr"].default is None
    assert "codebook" in inspect.signature(capi.WifiRx.irs_sweep).parameters
    assert capi.IRS_MAX_CODES == 1024
    assert isinstance(block.channel_model.irs_best, property)
    sig = inspect.signature(irs.dft_codebook).parameters
    assert list(sig) == ["scale", "los_b2r", "over", "bits"] and sig["los_b2r"].default is None and sig["over"].default == 1 and sig["bits"].default == 0
    sig = inspect.signature(irs.traverse_codebook).parameters
    assert list(sig) == ["scale", "interval", "irs_pos", "ap_pos", "accuracy", "freq", "bits"]
    assert sig["accuracy"].default == 10 and sig["freq"].default == 5e9 and sig["bits"].default == 0
    assert list(inspect.signature(irs.quantize).parameters) == ["psi", "bits"]


def test_config_and_constructor_checks():
    """IrsConfig(codebook=...) refuses what the entry point would, before a handle exists; the earlier checks are what they were"""
    from wifirx import block, irs
    geo = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))
    cb = irs.dft_codebook(4)
    c = irs.IrsConfig(**geo, codebook=cb, k_factor=10.0, pdp=(1.0, 0.5), refresh=100)
    assert c.n_elems == 16 and c.codebook.dtype == np.complex64 and c.codebook.shape == (16, 16) and c.codebook.flags.c_contiguous
    assert c.psi is None and c.align_bits == 0
    assert irs.IrsConfig(**geo, codebook=np.ones((1024, 16))).codebook.shape == (1024, 16)
    assert irs.IrsConfig(**geo, codebook=np.ones((1, 16), np.complex128)).codebook.dtype == np.complex64
    bad = [dict(geo, codebook=cb, psi=np.ones(16)), dict(geo, codebook=cb, align_bits=2), dict(geo, codebook=np.ones(16)),
           dict(geo, codebook=np.ones((4, 15))), dict(geo, codebook=np.ones((0, 16))), dict(geo, codebook=np.ones((1025, 16))),
           dict(geo, codebook=np.ones((2, 2, 16))), dict(geo, codebook=cb, k_factor=-1.0), dict(geo, codebook=cb, pdp=()),
           dict(geo, codebook=cb, refresh=0), dict(geo)]
    for kw in bad:
        with pytest.raises(ValueError):
            irs.IrsConfig(**kw)
    with pytest.raises(ValueError):
        block.channel_model(irs=c, taps=(1.0, 0.5))
    with pytest.raises(ValueError):
        block.channel_model(irs=c, doppler=1e-4)


@pytest.mark.gpu
def test_host_checks_queue_nothing():
    import ctypes as C
    from wifirx import capi
    rx = capi.WifiRx(max_sym=1, device=0)
    try:
        lib, N, L, K, n_sets = capi.lib(), 8, 2, 5, 3
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        words = n_sets * L * 2 + n_sets * K + n_sets + 16
        out = rx.alloc(words * 4).upload(np.full(words, 0x7FC0DEAD, np.uint32))
        canary = out.download(np.uint8, words * 4)
        taps_p, power_p = out.ptr, out.ptr + n_sets * L * 8
        best_p = power_p + n_sets * K * 4
        dev = rx.alloc(4096)                     # stands for a device codebook and scatter
        arr = dict(pdp=np.array([1.0, 0.5], np.float32), a=np.ones(N, np.complex64), b=np.ones(N, np.complex64),
                   d=np.ones(1, np.complex64), cb=np.ones((K, N), np.complex64))

        def call(**kw):
            v = dict(taps=taps_p, n_sets=n_sets, n_taps=L, pdp=P(arr["pdp"]), gain=1.0, n_elems=N, a=P(arr["a"]), b=P(arr["b"]),
                     d=P(arr["d"]), k=1.0, dg=1.0, cb=P(arr["cb"]), cb_dev=0, n_codes=K, scatter=None, n_scatter=0,
                     seed=1, best=best_p, power=power_p)
            v.update(kw)
            return lib.wifirx_irs_sweep(rx._h, v["taps"], v["n_sets"], v["n_taps"], v["pdp"], v["gain"], v["n_elems"], v["a"], v["b"],
                                        v["d"], v["k"], v["dg"], v["cb"], v["cb_dev"], v["n_codes"], v["scatter"],
                                        v["n_scatter"], v["seed"], v["best"], v["power"])

        def pdp(*v):
            keep.append(np.array(v, np.float32))
            return P(keep[-1])

        keep = []
        inf, nan = float("inf"), float("nan")
        cases = [
            # the new grounds
            dict(cb=None), dict(n_codes=0), dict(n_codes=1025), dict(taps=None, best=None, power=None),
            dict(taps=taps_p + 4), dict(power=power_p + 2), dict(best=best_p + 1), dict(cb=dev.ptr + 4, cb_dev=1),
            dict(cb=P(arr["cb"]).value + 2),
            # wifirx_irs_taps' grounds for the shared arguments
            dict(pdp=None), dict(a=None), dict(b=None), dict(d=None), dict(scatter=dev.ptr, n_scatter=0),
            dict(n_elems=0), dict(n_elems=4097), dict(n_taps=0), dict(n_taps=17, pdp=pdp(*([1.0] * 17))),
            dict(k=-1.0), dict(k=nan), dict(k=inf),
            dict(pdp=pdp(1.0, -0.5)), dict(pdp=pdp(nan, 1.0)), dict(pdp=pdp(1.0, inf)),
            dict(gain=nan), dict(gain=inf), dict(dg=nan), dict(dg=-inf),
            dict(scatter=dev.ptr + 4, n_scatter=1), dict(pdp=P(arr["pdp"]).value + 1),
            dict(a=P(arr["a"]).value + 2), dict(b=P(arr["b"]).value + 1), dict(d=P(arr["d"]).value + 2),
        ]
        for kw in cases:
            assert call(**kw) == capi.EINVAL, kw
        # every check comes before n_sets = 0 is looked at; n_sets = 0 itself does nothing
        assert call(n_sets=0, n_codes=0) == capi.EINVAL
        assert call(n_sets=0) == capi.OK
        rx.sync()
        assert out.download(np.uint8, words * 4).tobytes() == canary.tobytes(), "a refused call wrote"
        # what the checks let through: any one output alone, no direct path without los_b2u, one entry, a device codebook
        assert call(best=None, power=None) == capi.OK
        assert call(taps=None, power=None) == capi.OK
        assert call(taps=None, best=None, d=None, dg=0.0) == capi.OK
        dev.upload(np.ones(N, np.complex64))
        assert call(cb=dev.ptr, cb_dev=1, n_codes=1, k=0.0) == capi.OK
        rx.sync()
        assert np.isfinite(out.download(np.complex64, n_sets * L)).all()
        assert (out.download(np.uint8, words * 4)[n_sets * (L * 8 + K * 4):][:n_sets * 2].view(np.uint16) == 0).all()
        out.free()
        dev.free()
    finally:
        rx.close()
