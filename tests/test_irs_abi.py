"""wifirx_irs_taps in the C ABI and the Python surface: the declaration, the ctypes prototype and the constructor checks on a
box without a GPU; the host checks of the entry point, which need a handle, on the device."""
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm


def test_symbol_declared_exported_and_listed():
    from wifirx import capi
    assert re.search(r"\bint\s+wifirx_irs_taps\s*\(", _header())
    assert "wifirx_irs_taps" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_irs_taps")
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4          # additive: the version stays


def test_21_arguments_word_for_word():
    import ctypes as C
    from wifirx import capi
    want = ["wifirx_handle* h", "float* taps_out", "uint32_t n_sets", "uint32_t n_taps", "const float* pdp", "float gain",
            "uint32_t n_elems", "const float* los_b2r", "const float* los_r2u", "const float* los_b2u", "float k_factor",
            "float direct_gain", "const float* psi", "int psi_on_device", "uint32_t n_psi_sets", "uint32_t align_bits",
            "const float* scatter", "uint32_t n_scatter", "uint64_t irs_seed", "float* elems_out", "uint8_t* codes_out"]
    assert _norm(_decl(_header(), "wifirx_irs_taps")) == want
    kinds = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    types = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in want]
    assert list(capi.lib().wifirx_irs_taps.argtypes) == types


def test_header_comment_carries_the_rule():
    raw = _header_raw()
    at = raw.index("int  wifirx_irs_taps(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for word in ("NUMERICS.md rule 25", "(n, r, l, 2)", "0xFFFFFFFF", "(r L + l) % n_scatter", "r % n_psi_sets", "xor 32, 16, 8, 4, 2, 1",
                 "lowest c at a tie", "ORDER: as wifirx_channel", "WIFIRX_EINVAL"):
        assert word in comment, word


def test_python_surface():
    from wifirx import block, capi, irs
    prm = inspect.signature(capi.WifiRx.irs_taps_dev).parameters
    assert prm["k_factor"].default == 0.0 and prm["direct_gain"].default == 1.0 and prm["align_bits"].default == 0
    assert prm["scatter"].default is None and prm["seed"].default == 0
    assert hasattr(capi.WifiRx, "irs_taps")
    assert inspect.signature(block.channel_model.__init__).parameters["irs"].default is None
    assert hasattr(block.channel_model, "set_psi")
    assert capi.IRS_MAX_ELEMS == 4096 and capi.IRS_MAX_TAPS == 16
    assert irs.PHASES.dtype == np.complex64 and np.abs(irs.PHASES - np.exp(2j * np.pi * np.arange(8) / 8)).max() < 1e-7
    p = irs.random_psi(100, 2, 1)
    assert p.dtype == np.complex64 and set(np.round(p, 6).tolist()) <= {1, 1j, -1, -1j}
    assert np.array_equal(p, irs.random_psi(100, 2, 1)) and not np.array_equal(p, irs.random_psi(100, 2, 2))


def test_config_and_constructor_checks():
    """IrsConfig and channel_model(irs=...) refuse what the entry point would, before a handle exists"""
    from wifirx import block, irs
    geo = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))
    c = irs.IrsConfig(**geo, psi=np.ones(16), k_factor=10.0, pdp=(1.0, 0.5), refresh=100)
    assert c.n_elems == 16 and c.los_b2r.dtype == np.complex64 and c.los_b2u == 1.0 and c.pdp.dtype == np.float32
    assert irs.IrsConfig(los_b2r=np.ones(5), los_r2u=np.ones(5), direct_gain=0.0, align_bits=2).n_elems == 5
    bad = [dict(geo), dict(geo, psi=np.ones(15)), dict(geo, align_bits=4), dict(geo, align_bits=1, k_factor=-1.0),
           dict(geo, align_bits=1, k_factor=float("nan")), dict(geo, align_bits=1, pdp=()), dict(geo, align_bits=1, pdp=np.ones(17)),
           dict(geo, align_bits=1, pdp=(1.0, -0.1)), dict(geo, align_bits=1, refresh=0), dict(geo, align_bits=1, direct_gain=float("inf")),
           dict(scale=4, align_bits=1), dict(los_b2r=np.ones(5), align_bits=1), dict(los_b2r=np.ones(5), los_r2u=np.ones(6), align_bits=1),
           dict(los_b2r=np.ones(5), los_r2u=np.ones(5), align_bits=1),          # a direct path without los_b2u
           dict(los_b2r=np.ones(4097), los_r2u=np.ones(4097), direct_gain=0.0, align_bits=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            irs.IrsConfig(**kw)
    with pytest.raises(TypeError):
        block.channel_model(irs=dict(geo))
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
        lib, N, L, n_sets = capi.lib(), 8, 2, 3
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        out = rx.alloc(n_sets * L * 8 + 64).upload(np.full(n_sets * L * 2 + 16, 0x7FC0DEAD, np.uint32))
        canary = out.download(np.uint8, n_sets * L * 8 + 64)
        dev = rx.alloc(4096)                     # stands for device psi, scatter, elems_out, codes_out
        arr = dict(pdp=np.array([1.0, 0.5], np.float32), a=np.ones(N, np.complex64), b=np.ones(N, np.complex64),
                   d=np.ones(1, np.complex64), psi=np.ones(N, np.complex64))

        def call(**kw):
            v = dict(taps=out.ptr, n_sets=n_sets, n_taps=L, pdp=P(arr["pdp"]), gain=1.0, n_elems=N, a=P(arr["a"]), b=P(arr["b"]),
                     d=P(arr["d"]), k=1.0, dg=1.0, psi=P(arr["psi"]), psi_dev=0, n_psi=1, bits=0, scatter=None, n_scatter=0,
                     seed=1, elems=None, codes=None)
            v.update(kw)
            return lib.wifirx_irs_taps(rx._h, v["taps"], v["n_sets"], v["n_taps"], v["pdp"], v["gain"], v["n_elems"], v["a"], v["b"],
                                       v["d"], v["k"], v["dg"], v["psi"], v["psi_dev"], v["n_psi"], v["bits"], v["scatter"],
                                       v["n_scatter"], v["seed"], v["elems"], v["codes"])

        def pdp(*v):
            keep.append(np.array(v, np.float32))
            return P(keep[-1])

        keep = []
        inf, nan = float("inf"), float("nan")
        cases = [
            dict(taps=None), dict(pdp=None), dict(a=None), dict(b=None),
            dict(d=None),                                                    # a direct path without its line of sight
            dict(psi=None), dict(n_psi=0), dict(scatter=dev.ptr, n_scatter=0),
            dict(n_elems=0), dict(n_elems=4097), dict(n_taps=0), dict(n_taps=17, pdp=pdp(*([1.0] * 17))),
            dict(bits=4), dict(codes=dev.ptr),                               # codes_out with align_bits = 0
            dict(k=-1.0), dict(k=nan), dict(k=inf),
            dict(pdp=pdp(1.0, -0.5)), dict(pdp=pdp(nan, 1.0)), dict(pdp=pdp(1.0, inf)),
            dict(gain=nan), dict(gain=inf), dict(dg=nan), dict(dg=-inf),
            dict(taps=out.ptr + 4), dict(scatter=dev.ptr + 4, n_scatter=1), dict(elems=dev.ptr + 4),
            dict(psi=dev.ptr + 4, psi_dev=1), dict(psi=P(arr["psi"]).value + 2), dict(pdp=P(arr["pdp"]).value + 1),
            dict(a=P(arr["a"]).value + 2), dict(b=P(arr["b"]).value + 1), dict(d=P(arr["d"]).value + 2),
        ]
        for kw in cases:
            assert call(**kw) == capi.EINVAL, kw
        # every check comes before n_sets = 0 is looked at; n_sets = 0 itself does nothing
        assert call(n_sets=0, n_elems=0) == capi.EINVAL
        assert call(n_sets=0) == capi.OK
        rx.sync()
        assert out.download(np.uint8, n_sets * L * 8 + 64).tobytes() == canary.tobytes(), "a refused call wrote taps"
        # what the checks let through: no direct path without los_b2u, aligned mode without psi, the largest sizes
        assert call(d=None, dg=0.0) == capi.OK
        assert call(psi=None, n_psi=0, bits=3, codes=dev.ptr) == capi.OK
        assert call(k=0.0, a=P(arr["a"]), pdp=pdp(0.0, 0.0)) == capi.OK
        rx.sync()
        assert np.isfinite(out.download(np.complex64, n_sets * L)).all()
        out.free()
        dev.free()
    finally:
        rx.close()
