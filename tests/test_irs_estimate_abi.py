"""wifirx_irs_estimate in the C ABI and the Python surface: the declaration, the ctypes prototype and the helpers on a box without
a GPU; the host checks of the entry point, which need a handle, on the device."""
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm

WANT = ["wifirx_handle* h", "float* taps_out", "uint32_t n_ant", "uint32_t n_sets", "uint32_t n_taps", "const float* pdp",
        "float gain", "uint32_t n_elems", "const float* los_b2r", "const float* los_r2u", "const float* los_b2u", "float k_factor",
        "float direct_gain", "const float* pilot", "int pilot_on_device", "uint32_t n_pilots", "uint32_t n_groups",
        "const uint16_t* group", "float noise_sigma", "float est_scale", "uint32_t align_bits", "const float* scatter",
        "uint32_t n_scatter", "const float* noise", "uint32_t n_noise", "uint64_t irs_seed", "float* est_out", "uint8_t* codes_out",
        "float* obs_out"]


def test_symbol_declared_exported_and_listed():
    from wifirx import capi
    assert re.search(r"\bint\s+wifirx_irs_estimate\s*\(", _header())
    assert "wifirx_irs_estimate" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_irs_estimate")
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4          # additive: the version stays


def test_29_arguments_word_for_word():
    import ctypes as C
    from wifirx import capi
    assert _norm(_decl(_header(), "wifirx_irs_estimate")) == WANT
    kinds = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    types = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in WANT]
    assert list(capi.lib().wifirx_irs_estimate.argtypes) == types
    # the shared arguments are wifirx_irs_taps_multi's, in its order
    assert WANT[:13] == _norm(_decl(_header(), "wifirx_irs_taps_multi"))[:13]


def test_header_comment_carries_the_rule():
    raw = _header_raw()
    at = raw.index("int  wifirx_irs_estimate(")
    comment = raw[raw.rindex("/* The surface configured", 0, at):at]
    for word in ("NUMERICS.md rule 29", "Channel.CH_est", "(t, r, rho, 3)", "(r R + rho) % n_noise", "pilot[t][group[n]]",
                 "one fma chain", "from +0", "multiple of 4", "v_mfma_f32_16x16x4_f32", "conj(p_{t,j})", "p_{t,0} = 1",
                 "lowest c wins a tie", "wifirx_irs_taps_multi", "bit for bit", "1 <= n_pilots <= 1024", "min(N, 1023)",
                 "1 / (T + sigma^2)", "all four outputs NULL", "At most three", "ORDER: as wifirx_channel", "WIFIRX_EINVAL",
                 "WIFIRX_ERANGE"):
        assert word in comment, word


def test_python_surface():
    from wifirx import capi, irs
    prm = inspect.signature(capi.WifiRx.irs_estimate_dev).parameters
    assert list(prm)[:7] == ["self", "taps_ptr", "n_sets", "pdp", "los_b2r", "los_r2u", "los_b2u"]
    for name, default in dict(n_pilots=None, n_groups=None, group=None, sigma=0.0, est_scale=None, align_bits=0, gain=1.0,
                              k_factor=0.0, direct_gain=1.0, scatter=None, n_scatter=None, noise=None, n_noise=None, seed=0,
                              est_ptr=None, codes_ptr=None, obs_ptr=None).items():
        assert prm[name].default == default and prm[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert prm["pilots"].kind is inspect.Parameter.KEYWORD_ONLY and prm["pilots"].default is inspect.Parameter.empty
    prm = inspect.signature(capi.WifiRx.irs_estimate).parameters
    assert prm["want"].default == ("taps", "est", "codes", "obs") and prm["pilots"].default is inspect.Parameter.empty
    assert (capi.IRS_MAX_PILOTS, capi.IRS_MAX_GROUPS) == (1024, 1023)
    assert list(inspect.signature(irs.dft_pilots).parameters) == ["n_groups"]
    assert list(inspect.signature(irs.hadamard_pilots).parameters) == ["n_groups"]
    assert list(inspect.signature(irs.groups).parameters) == ["scale", "c"]
    sig = inspect.signature(irs.est_scale).parameters
    assert list(sig) == ["n_pilots", "sigma", "mmse"] and sig["sigma"].default == 0.0 and sig["mmse"].default is False


def test_config_and_constructor_checks():
    """IrsConfig(pilots=...) refuses what the entry point would, before a handle exists; the earlier checks are what they were"""
    from wifirx import block, irs
    geo = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))
    c = irs.IrsConfig(**geo, pilots=irs.hadamard_pilots(4), group=irs.groups(4, 2), pilot_sigma=0.5, pilot_bits=2, pdp=(1.0, 0.5))
    assert c.pilots.dtype == np.complex64 and c.pilots.shape == (8, 4) and c.pilots.flags.c_contiguous
    assert c.group.dtype == np.uint16 and c.group.shape == (16,) and c.pilot_sigma == 0.5 and c.pilot_bits == 2
    assert c.psi is None and c.align_bits == 0 and c.codebook is None
    assert irs.IrsConfig(**geo, pilots=irs.dft_pilots(16)).pilot_bits == 2 and irs.IrsConfig(**geo, pilots=irs.dft_pilots(16)).group is None
    assert isinstance(block.channel_model.irs_codes, property)
    pl = irs.dft_pilots(16)
    bad = [dict(geo, pilots=pl, codebook=irs.dft_codebook(4)), dict(geo, pilots=pl, align_bits=2), dict(geo, pilots=pl, psi=np.ones(16)),
           dict(geo, pilots=np.ones(16)), dict(geo, pilots=np.ones((1025, 16))), dict(geo, pilots=np.ones((0, 16))),
           dict(geo, pilots=np.ones((4, 17))), dict(geo, pilots=np.ones((4, 4))), dict(geo, pilots=pl, group=np.arange(16)[:15]),
           dict(geo, pilots=irs.hadamard_pilots(4), group=np.full(16, 4)), dict(geo, pilots=pl, pilot_sigma=-1.0),
           dict(geo, pilots=pl, pilot_sigma=float("nan")), dict(geo, pilots=pl, pilot_bits=0), dict(geo, pilots=pl, pilot_bits=4),
           dict(geo, group=irs.groups(4, 2), psi=np.ones(16)), dict(geo, pilots=pl, est_scale=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            irs.IrsConfig(**kw)


@pytest.mark.gpu
def test_host_checks_queue_nothing():
    import ctypes as C
    from wifirx import capi
    rx = capi.WifiRx(max_sym=1, device=0)
    try:
        lib, M, N, L, T, G, n_sets = capi.lib(), 2, 8, 2, 5, 4, 3
        R = M * L
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        sizes = [M * n_sets * L * 8, n_sets * R * (G + 1) * 8, n_sets * R * T * 8, n_sets * G + 64]
        total = sum(sizes)
        out = rx.alloc(total).upload(np.full(total // 4, 0x7FC0DEAD, np.uint32))
        canary = out.download(np.uint8, total)
        taps_p = out.ptr
        est_p, obs_p, codes_p = taps_p + sizes[0], taps_p + sizes[0] + sizes[1], taps_p + sizes[0] + sizes[1] + sizes[2]
        dev = rx.alloc(4096)                     # stands for a device pilot, scatter and noise
        arr = dict(pdp=np.array([1.0, 0.5], np.float32), a=np.ones((M, N), np.complex64), b=np.ones(N, np.complex64),
                   d=np.ones(M, np.complex64), pl=np.ones((T, G), np.complex64), grp=(np.arange(N) % G).astype(np.uint16),
                   grp8=np.arange(N + 1).astype(np.uint16))
        keep = []

        def pdp(*v):
            keep.append(np.array(v, np.float32))
            return P(keep[-1])

        def grp(*v):
            keep.append(np.array(v, np.uint16))
            return P(keep[-1])

        def call(**kw):
            v = dict(taps=taps_p, n_ant=M, n_sets=n_sets, n_taps=L, pdp=P(arr["pdp"]), gain=1.0, n_elems=N, a=P(arr["a"]),
                     b=P(arr["b"]), d=P(arr["d"]), k=1.0, dg=1.0, pl=P(arr["pl"]), pl_dev=0, T=T, G=G, grp=P(arr["grp"]), sigma=0.5,
                     kappa=0.2, bits=2, scatter=None, n_scatter=0, noise=None, n_noise=0, seed=1, est=est_p, codes=codes_p, obs=obs_p)
            v.update(kw)
            return lib.wifirx_irs_estimate(rx._h, v["taps"], v["n_ant"], v["n_sets"], v["n_taps"], v["pdp"], v["gain"], v["n_elems"],
                                           v["a"], v["b"], v["d"], v["k"], v["dg"], v["pl"], v["pl_dev"], v["T"], v["G"], v["grp"],
                                           v["sigma"], v["kappa"], v["bits"], v["scatter"], v["n_scatter"], v["noise"], v["n_noise"],
                                           v["seed"], v["est"], v["codes"], v["obs"])

        inf, nan = float("inf"), float("nan")
        cases = [
            # the new grounds
            dict(pl=None), dict(T=0), dict(T=1025), dict(G=0), dict(G=N + 1, grp=None), dict(G=1024, n_elems=4096),
            dict(grp=None), dict(grp=grp(0, 1, 2, 3, 4, 1, 2, 3)), dict(sigma=-0.5), dict(sigma=nan), dict(sigma=inf),
            dict(kappa=nan), dict(kappa=inf), dict(noise=dev.ptr, n_noise=0), dict(bits=4), dict(bits=0),
            dict(bits=0, taps=None), dict(bits=0, codes=None), dict(taps=None, est=None, codes=None, obs=None),
            dict(taps=taps_p + 4), dict(est=est_p + 4), dict(obs=obs_p + 4), dict(noise=dev.ptr + 4, n_noise=1),
            dict(pl=dev.ptr + 4, pl_dev=1), dict(pl=P(arr["pl"]).value + 2), dict(grp=P(arr["grp8"]).value + 1),
            # wifirx_irs_taps_multi's grounds for the shared arguments
            dict(n_ant=0), dict(n_ant=9), dict(pdp=None), dict(a=None), dict(b=None), dict(d=None), dict(scatter=dev.ptr, n_scatter=0),
            dict(n_elems=0), dict(n_elems=4097), dict(n_taps=0), dict(n_taps=17, pdp=pdp(*([1.0] * 17))),
            dict(k=-1.0), dict(k=nan), dict(k=inf),
            dict(pdp=pdp(1.0, -0.5)), dict(pdp=pdp(nan, 1.0)), dict(pdp=pdp(1.0, inf)),
            dict(gain=nan), dict(gain=inf), dict(dg=nan), dict(dg=-inf),
            dict(scatter=dev.ptr + 4, n_scatter=1), dict(pdp=P(arr["pdp"]).value + 1),
            dict(a=P(arr["a"]).value + 2), dict(b=P(arr["b"]).value + 1), dict(d=P(arr["d"]).value + 2),
        ]
        for kw in cases:
            assert call(**kw) == capi.EINVAL, kw
        # every check comes before n_sets = 0 is looked at; n_sets = 0 itself does nothing; too many sets are out of range
        assert call(n_sets=0, T=0) == capi.EINVAL
        assert call(n_sets=0) == capi.OK
        assert call(n_sets=1 << 31) == capi.ERANGE
        rx.sync()
        assert out.download(np.uint8, total).tobytes() == canary.tobytes(), "a refused call wrote"
        # what the checks let through: any one output alone, no decision without taps and codes, the identity map, no direct
        # path without los_b2u, a device pilot, any finite scale
        assert call(est=None, codes=None, obs=None) == capi.OK
        assert call(taps=None, codes=None, obs=None, bits=0) == capi.OK
        assert call(taps=None, est=None, obs=None) == capi.OK
        assert call(taps=None, est=None, codes=None, bits=0, sigma=0.0) == capi.OK
        keep.append(np.ones((T, N), np.complex64))
        assert call(G=N, grp=None, pl=P(keep[-1]), d=None, dg=0.0, kappa=-3.0, est=None, codes=None) == capi.OK   # (G + 1 and G wider)
        dev.upload(np.ones(T * G, np.complex64))
        assert call(pl=dev.ptr, pl_dev=1, k=0.0) == capi.OK
        rx.sync()
        assert np.isfinite(out.download(np.complex64, (sizes[0] + sizes[1] + sizes[2]) // 8)).all()
        assert (out.download(np.uint8, total)[total - sizes[3]:][:n_sets * G] < 4).all()
        assert (out.download(np.uint8, total)[total - 64:] == canary[total - 64:]).all()
        out.free()
        dev.free()
    finally:
        rx.close()
