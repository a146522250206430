"""wifirx_irs_optimize_weighted in the C ABI and the Python surface: the declaration, the ctypes prototype, the header comment and
the configuration on a box without a GPU; the host checks of the entry point, which need a handle, on the device."""
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm

WANT = ["wifirx_handle* h", "const float* coef", "uint32_t n_sets", "uint32_t n_rows", "uint32_t n_cols", "const float* weight",
        "int weight_on_device", "uint32_t n_weight_sets", "uint32_t bits", "uint32_t max_sweeps", "int start", "int direct_blocked",
        "const uint8_t* codes_in", "uint32_t n_elems", "const uint16_t* group", "uint8_t* codes_out", "float* psi_out",
        "float* power_out", "uint8_t* sweeps_out"]
GEO = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))


def test_symbol_declared_exported_and_listed():
    from wifirx import capi
    hdr = _header()
    assert re.search(r"\bint\s+wifirx_irs_optimize_weighted\s*\(", hdr)
    assert "wifirx_irs_optimize_weighted" in capi.EXPORTS and hasattr(capi.lib(), "wifirx_irs_optimize_weighted")
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4          # additive: the version stays
    # the new declaration stands behind the old one, which is what it was
    assert hdr.index("wifirx_irs_optimize(") < hdr.index("wifirx_irs_optimize_weighted(")
    assert len(_norm(_decl(hdr, "wifirx_irs_optimize"))) == 16


def test_19_arguments_word_for_word():
    import ctypes as C
    from wifirx import capi
    assert _norm(_decl(_header(), "wifirx_irs_optimize_weighted")) == WANT
    kinds = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    types = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in WANT]
    assert list(capi.lib().wifirx_irs_optimize_weighted.argtypes) == types


def test_header_comment_carries_the_rule():
    raw = _header_raw()
    at = raw.index("int  wifirx_irs_optimize_weighted(")
    comment = raw[raw.rindex("/* The joint phase decision with a real weight", 0, at):at]
    for word in ("NUMERICS.md rule 31", "P_w = sum_rho w_rho", "either sign", "w_rho == 0", "either sign of zero", "+0, selected and not multiplied",
                 "still carried", "tw_rho = (w_rho t.re, w_rho t.im)", "one float32 multiply", "no fma", "tw_i + tw_{i+64}",
                 "absent rows are +0", "lane xor 32, 16, 8, 4, 2, 1", "w_rho q_rho", "may be negative", "WIFIRX_IRS_START_REF",
                 "whatever w_0 is", "stays", "bit for bit", "2^k", "weight_on_device", "n_weight_sets", "r % n_weight_sets",
                 "not inspected", "non-finite host weight", "One kernel launch per call", "ORDER: as wifirx_channel",
                 "WIFIRX_EINVAL", "WIFIRX_ERANGE"):
        assert word in comment, word
    # the sentence of wifirx_irs_optimize that said weights are not offered now names the call
    at = raw.index("int  wifirx_irs_optimize(")
    assert "wifirx_irs_optimize_weighted" in raw[raw.rindex("/* The joint phase decision", 0, at):at]


def test_python_surface():
    from wifirx import capi, irs
    prm = inspect.signature(capi.WifiRx.irs_optimize_dev).parameters
    for name, default in dict(weights=None, weights_ptr=None, n_weight_sets=1).items():
        assert prm[name].default == default and prm[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    prm = inspect.signature(capi.WifiRx.irs_optimize).parameters
    assert prm["weights"].default is None and prm["weights"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(irs.row_weights).parameters) == ["antennas", "taps", "tap", "ant"]
    prm = inspect.signature(irs.tap_weights).parameters
    assert list(prm) == ["taps", "keep", "penalty"] and prm["keep"].default == 1 and prm["penalty"].default == 0.0


def test_weight_helpers():
    from wifirx import irs
    assert irs.tap_weights(4).tolist() == [1, 0, 0, 0] and irs.tap_weights(4).dtype == np.float32
    assert irs.tap_weights(3, keep=2, penalty=0.5).tolist() == [1, 1, -0.5]
    assert irs.tap_weights(2, keep=0, penalty=1).tolist() == [-1, -1]
    w = irs.row_weights(2, 3, tap=(1, 0, -1), ant=(1, 0.25))
    assert w.dtype == np.float32 and w.tolist() == [1, 0, -1, 0.25, 0, -0.25]            # w_{m L + l} = ant[m] tap[l]
    assert irs.row_weights(2, 2).tolist() == [1, 1, 1, 1] and irs.row_weights(2, 2, ant=(2, 3)).tolist() == [2, 2, 3, 3]
    assert irs.row_weights(2, 2, tap=irs.tap_weights(2)).tolist() == [1, 0, 1, 0]
    for bad in (lambda: irs.row_weights(2, 3, tap=(1, 0)), lambda: irs.row_weights(2, 3, ant=(1,)), lambda: irs.row_weights(0, 1),
                lambda: irs.tap_weights(2, keep=3), lambda: irs.tap_weights(0)):
        with pytest.raises(ValueError):
            bad()


def test_config_checks():
    """IrsConfig(tap_weights=..., ant_weights=...) before a handle exists; with both None the configuration is what it was"""
    from wifirx import irs
    pl = irs.dft_pilots(16)
    c = irs.IrsConfig(**GEO, pilots=pl, decision="joint")
    assert c.tap_weights is None and c.ant_weights is None and c.row_weights is None
    c = irs.IrsConfig(**GEO, pilots=pl, decision="joint", pdp=(0.6, 0.3, 0.1), antennas=2, tap_weights=(1, 0, -0.5))
    assert c.row_weights.tolist() == [1, 0, -0.5, 1, 0, -0.5]
    c = irs.IrsConfig(**GEO, pilots=pl, decision="joint", pdp=(0.6, 0.4), antennas=2, ant_weights=(1, 0.25))
    assert c.row_weights.tolist() == [1, 1, 0.25, 0.25]
    for kw in (dict(tap_weights=(1,)), dict(decision="ref", tap_weights=(1,)), dict(ant_weights=(1,)),       # weights without joint
               dict(decision="joint", tap_weights=(1, 0)), dict(decision="joint", ant_weights=(1, 1)),         # a wrong length
               dict(decision="joint", pdp=(0.5, 0.5), tap_weights=(1, 0, 0)),
               dict(decision="joint", tap_weights=(np.nan,)), dict(decision="joint", ant_weights=(np.inf,)),   # not finite
               dict(decision="best")):                                                                        # still refused
        with pytest.raises(ValueError):
            irs.IrsConfig(**GEO, pilots=pl, **kw)


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
        wdev = rx.alloc(n_sets * R * 4 + 64).upload(np.ones(n_sets * R + 16, np.float32))
        grp, grp9 = (np.arange(N) % G).astype(np.uint16), np.arange(N + 1).astype(np.uint16)
        w_host, w9 = np.linspace(-1, 1, R).astype(np.float32), np.ones(R + 1, np.float32)
        keep = []

        def g16(*v):
            keep.append(np.array(v, np.uint16))
            return P(keep[-1])

        def f32(*v):
            keep.append(np.array(v, np.float32))
            return P(keep[-1])

        def call(**kw):
            v = dict(coef=coef.ptr, n_sets=n_sets, R=R, J=J, w=P(w_host), on_dev=0, nws=1, bits=2, S=S, start=capi.IRS_START_REF,
                     blocked=0, cin=None, N=N, grp=P(grp), codes=codes_p, psi=psi_p, power=power_p, sweeps=sweeps_p)
            v.update(kw)
            return lib.wifirx_irs_optimize_weighted(rx._h, v["coef"], v["n_sets"], v["R"], v["J"], v["w"], v["on_dev"], v["nws"],
                                                    v["bits"], v["S"], v["start"], v["blocked"], v["cin"], v["N"], v["grp"],
                                                    v["codes"], v["psi"], v["power"], v["sweeps"])

        # everything wifirx_irs_optimize checks
        cases = [dict(coef=None), dict(codes=None, psi=None), dict(R=0), dict(R=129), dict(J=1), dict(J=0), dict(J=1025),
                 dict(bits=0), dict(bits=4), dict(S=17), dict(start=3), dict(start=-1), dict(start=capi.IRS_START_GIVEN),
                 dict(N=0), dict(N=4097, grp=None), dict(grp=None), dict(N=G + 1, grp=None), dict(grp=g16(0, 1, 2, 3, 4, 0, 1, 2)),
                 dict(coef=coef.ptr + 4), dict(psi=psi_p + 4), dict(power=power_p + 2), dict(grp=P(grp9).value + 1)]
        # the weights: NULL, n_weight_sets outside {1, n_sets}, != 1 with host weights, a non-finite host weight, misaligned
        cases += [dict(w=None), dict(w=None, on_dev=1), dict(nws=0), dict(nws=2), dict(nws=n_sets), dict(w=wdev.ptr, on_dev=1, nws=2),
                  dict(w=wdev.ptr, on_dev=1, nws=0), dict(w=wdev.ptr, on_dev=1, nws=n_sets + 1),
                  dict(w=f32(1, 1, np.nan, 1, 1, 1)), dict(w=f32(1, 1, 1, 1, 1, np.inf)), dict(w=f32(-np.inf, 1, 1, 1, 1, 1)),
                  dict(w=wdev.ptr + 2, on_dev=1), dict(w=wdev.ptr + 1, on_dev=1, nws=n_sets), dict(w=P(w9).value + 2)]
        for kw in cases:
            assert call(**kw) == capi.EINVAL, kw
        # every check comes before n_sets = 0 is looked at; n_sets = 0 itself does nothing; too many sets are out of range
        assert call(n_sets=0, bits=0) == capi.EINVAL
        assert call(n_sets=0, w=None) == capi.EINVAL
        assert call(n_sets=0) == capi.OK
        assert call(n_sets=0, w=wdev.ptr, on_dev=1) == capi.OK
        assert call(n_sets=1 << 31) == capi.ERANGE
        assert call(n_sets=1 << 31, w=wdev.ptr, on_dev=1) == capi.ERANGE
        rx.sync()
        assert out.download(np.uint8, total).tobytes() == canary.tobytes(), "a refused call wrote"
        # what the checks let through: host weights with and without the group map, device weights of one block and of one
        # block per set (4-byte aligned is enough), given codes, the ends of the ranges
        assert call(psi=None, power=None, sweeps=None, N=0, grp=None) == capi.OK
        assert call(codes=None) == capi.OK
        assert call(w=wdev.ptr + 4, on_dev=1) == capi.OK
        assert call(w=wdev.ptr, on_dev=1, nws=n_sets) == capi.OK
        assert call(N=G, grp=None, start=capi.IRS_START_GIVEN, cin=cin.ptr, S=0, bits=1, blocked=1) == capi.OK
        assert call(start=capi.IRS_START_ZERO, S=4, bits=3, w=f32(0, -0.0, 1e30, -1e-30, 1, 1)) == capi.OK
        rx.sync()
        got = out.download(np.uint8, total)
        assert (got[sizes[0] + sizes[1]:][:n_sets * G] < 8).all()
        assert (got[total - 64 + n_sets:] == canary[total - 64 + n_sets:]).all()
        for b in (out, coef, cin, wdev):
            b.free()
    finally:
        rx.close()
