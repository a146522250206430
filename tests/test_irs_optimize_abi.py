"""wifirx_irs_optimize in the C ABI and the Python surface: the declaration, the ctypes prototype and the configuration on a box
without a GPU; the host checks of the entry point, which need a handle, on the device."""
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm

WANT = ["wifirx_handle* h", "const float* coef", "uint32_t n_sets", "uint32_t n_rows", "uint32_t n_cols", "uint32_t bits",
        "uint32_t max_sweeps", "int start", "int direct_blocked", "const uint8_t* codes_in", "uint32_t n_elems",
        "const uint16_t* group", "uint8_t* codes_out", "float* psi_out", "float* power_out", "uint8_t* sweeps_out"]


def test_symbol_declared_exported_and_listed():
    from wifirx import capi
    assert re.search(r"\bint\s+wifirx_irs_optimize\s*\(", _header())
    assert "wifirx_irs_optimize" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_irs_optimize")
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4          # additive: the version stays
    raw = _header_raw()
    for name, value in (("REF", 0), ("GIVEN", 1), ("ZERO", 2)):
        assert re.search(r"#define\s+WIFIRX_IRS_START_%s\s+%d\b" % (name, value), raw)
    assert (capi.IRS_START_REF, capi.IRS_START_GIVEN, capi.IRS_START_ZERO) == (0, 1, 2)
    assert capi.IRS_STARTS == {"ref": 0, "given": 1, "zero": 2}


def test_16_arguments_word_for_word():
    import ctypes as C
    from wifirx import capi
    assert _norm(_decl(_header(), "wifirx_irs_optimize")) == WANT
    kinds = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    types = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in WANT]
    assert list(capi.lib().wifirx_irs_optimize.argtypes) == types


def test_header_comment_carries_the_rule():
    raw = _header_raw()
    at = raw.index("int  wifirx_irs_optimize(")
    comment = raw[raw.rindex("/* The joint phase decision", 0, at):at]
    for word in ("NUMERICS.md rule 30", "coordinate ascent", "est_out", "WIFIRX_IRS_START_REF", "WIFIRX_IRS_START_GIVEN",
                 "WIFIRX_IRS_START_ZERO", "formed once, never recomputed", "t_i + t_{i+64}", "absent rows are +0",
                 "lane xor 32, 16, 8, 4, 2, 1", "strict >", "lowest c wins a tie", "NaN never replaces", "stays as it was",
                 "repeat the last value", "direct_blocked", "1 <= n_rows <= 128", "2 <= n_cols <= 1024", "0..16",
                 "wifirx_irs_taps_multi", "One kernel launch per call", "ORDER: as wifirx_channel", "WIFIRX_EINVAL", "WIFIRX_ERANGE"):
        assert word in comment, word
    # the sentences that said a joint decision is not offered now name the call
    for fn in ("wifirx_irs_taps_multi", "wifirx_irs_estimate"):
        at = raw.index("int  %s(" % fn)
        assert "wifirx_irs_optimize" in raw[raw.rindex("/*", 0, at):at], fn


def test_python_surface():
    from wifirx import capi
    prm = inspect.signature(capi.WifiRx.irs_optimize_dev).parameters
    assert list(prm)[:5] == ["self", "coef_ptr", "n_sets", "n_rows", "n_cols"]
    for name, default in dict(bits=2, max_sweeps=4, start="ref", direct_blocked=False, codes_in=None, n_elems=None, group=None,
                              codes_ptr=None, psi_ptr=None, power_ptr=None, sweeps_ptr=None).items():
        assert prm[name].default == default and prm[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    prm = inspect.signature(capi.WifiRx.irs_optimize).parameters
    assert list(prm)[:2] == ["self", "coef"] and prm["want"].default == ("codes", "psi", "power", "sweeps")
    assert prm["max_sweeps"].default == 4 and prm["start"].default == "ref"
    assert (capi.IRS_MAX_ROWS, capi.IRS_MAX_SWEEPS) == (128, 16)


def test_config_checks():
    """IrsConfig(decision=...) before a handle exists; decision="ref" is the default and leaves the configuration as it was"""
    from wifirx import irs
    geo = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))
    pl = irs.dft_pilots(16)
    c = irs.IrsConfig(**geo, pilots=pl)
    assert c.decision == "ref" and c.sweeps == 4
    c = irs.IrsConfig(**geo, pilots=irs.hadamard_pilots(4), group=irs.groups(4, 2), decision="joint", sweeps=7, antennas=4)
    assert c.decision == "joint" and c.sweeps == 7
    assert irs.IrsConfig(**geo, pilots=pl, decision="joint", sweeps=0).sweeps == 0
    for kw in (dict(geo, decision="joint"), dict(geo, align_bits=2, decision="joint"), dict(geo, pilots=pl, decision="best"),
               dict(geo, pilots=pl, decision="joint", sweeps=17), dict(geo, pilots=pl, decision="joint", sweeps=-1),
               dict(geo, codebook=irs.dft_codebook(4), decision="joint")):
        with pytest.raises(ValueError):
            irs.IrsConfig(**kw)


@pytest.mark.gpu
def test_host_checks_queue_nothing():
    import ctypes as C
    from wifirx import capi
    rx = capi.WifiRx(max_sym=1, device=0)
    try:
        lib, n_sets, R, J, N, S = capi.lib(), 3, 6, 5, 8, 4
        G = J - 1
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        sizes = [n_sets * N * 8, n_sets * (S + 1) * 4, n_sets * G, 64]         # psi, power, codes, sweeps + tail
        total = sum(sizes)
        out = rx.alloc(total).upload(np.full(total // 4, 0x7FC0DEAD, np.uint32))
        canary = out.download(np.uint8, total)
        psi_p, power_p, codes_p = out.ptr, out.ptr + sizes[0], out.ptr + sizes[0] + sizes[1]
        sweeps_p = codes_p + sizes[2]
        coef = rx.alloc(n_sets * R * J * 8 + 64).upload(np.ones(n_sets * R * J + 8, np.complex64))
        cin = rx.alloc(64).upload(np.zeros(64, np.uint8))
        grp, grp9 = (np.arange(N) % G).astype(np.uint16), np.arange(N + 1).astype(np.uint16)
        keep = []

        def g16(*v):
            keep.append(np.array(v, np.uint16))
            return P(keep[-1])

        def call(**kw):
            v = dict(coef=coef.ptr, n_sets=n_sets, R=R, J=J, bits=2, S=S, start=capi.IRS_START_REF, blocked=0, cin=None, N=N,
                     grp=P(grp), codes=codes_p, psi=psi_p, power=power_p, sweeps=sweeps_p)
            v.update(kw)
            return lib.wifirx_irs_optimize(rx._h, v["coef"], v["n_sets"], v["R"], v["J"], v["bits"], v["S"], v["start"],
                                           v["blocked"], v["cin"], v["N"], v["grp"], v["codes"], v["psi"], v["power"], v["sweeps"])

        cases = [dict(coef=None), dict(codes=None, psi=None), dict(R=0), dict(R=129), dict(J=1), dict(J=0), dict(J=1025),
                 dict(bits=0), dict(bits=4), dict(S=17), dict(start=3), dict(start=-1), dict(start=capi.IRS_START_GIVEN),
                 dict(N=0), dict(N=4097, grp=None), dict(grp=None), dict(N=G + 1, grp=None), dict(grp=g16(0, 1, 2, 3, 4, 0, 1, 2)),
                 dict(coef=coef.ptr + 4), dict(psi=psi_p + 4), dict(power=power_p + 2), dict(grp=P(grp9).value + 1)]
        for kw in cases:
            assert call(**kw) == capi.EINVAL, kw
        # every check comes before n_sets = 0 is looked at; n_sets = 0 itself does nothing; too many sets are out of range
        assert call(n_sets=0, bits=0) == capi.EINVAL
        assert call(n_sets=0) == capi.OK
        assert call(n_sets=1 << 31) == capi.ERANGE
        rx.sync()
        assert out.download(np.uint8, total).tobytes() == canary.tobytes(), "a refused call wrote"
        # what the checks let through: either of the two code outputs alone, the group map and n_elems unlooked at without
        # psi_out, the identity map, given codes, the ends of the ranges
        assert call(psi=None, power=None, sweeps=None, N=0, grp=None) == capi.OK
        assert call(codes=None) == capi.OK
        assert call(N=G, grp=None, start=capi.IRS_START_GIVEN, cin=cin.ptr, S=0, bits=1, blocked=1) == capi.OK
        assert call(start=capi.IRS_START_ZERO, S=4, bits=3) == capi.OK
        rx.sync()
        got = out.download(np.uint8, total)
        assert (got[sizes[0] + sizes[1]:][:n_sets * G] < 8).all()
        assert (got[total - 64 + n_sets:] == canary[total - 64 + n_sets:]).all()
        for b in (out, coef, cin):
            b.free()
    finally:
        rx.close()
