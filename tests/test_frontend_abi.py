"""The receive front end (NUMERICS.md rule 32) in the C ABI and the Python surface, on a box without a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np

from abi_helpers import ROOT, _decl, _header, _header_raw, _norm

import frontend_ref as fr

NAMES = (("wifirx_frontend", 8), ("wifirx_frontend_estimate", 4), ("wifirx_rx_impair", 7), ("wifirx_stream_frontend", 3),
         ("wifirx_stream_frontend_state", 2))


def test_declared_exported_and_bound():
    from wifirx import capi
    txt = _header()
    for name, n_args in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
        assert len(_decl(txt, name).split(",")) == n_args == len(getattr(capi.lib(), name).argtypes), name


def test_argument_lists():
    txt = _header()
    assert _norm(_decl(txt, "wifirx_frontend")) == ["wifirx_handle* h", "const wifirx_frontend_cfg* cfg", "wifirx_frontend_state* state_dev",
                                                    "const void* in", "int fmt", "float scale", "uint64_t n", "float* out"]
    assert _norm(_decl(txt, "wifirx_frontend_estimate")) == ["const wifirx_frontend_cfg* cfg", "const wifirx_frontend_state* state_host",
                                                             "float dc[2]", "float w[2]"]
    assert _norm(_decl(txt, "wifirx_rx_impair")) == ["wifirx_handle* h", "const float* in", "float* out", "uint64_t n", "const float mu[2]",
                                                     "const float nu[2]", "const float dc[2]"]
    assert _norm(_decl(txt, "wifirx_stream_frontend")) == ["wifirx_handle* h", "const wifirx_frontend_cfg* cfg", "const wifirx_frontend_state* init"]
    assert _norm(_decl(txt, "wifirx_stream_frontend_state")) == ["wifirx_handle* h", "wifirx_frontend_state* out_host"]


def test_ctypes_signatures():
    from wifirx import capi
    lib = capi.lib()
    assert list(lib.wifirx_frontend.argtypes) == [C.c_void_p, C.POINTER(capi.FrontendCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                                  C.c_uint64, C.c_void_p]
    assert list(lib.wifirx_stream_frontend.argtypes) == [C.c_void_p, C.POINTER(capi.FrontendCfg), C.c_void_p]
    assert list(lib.wifirx_rx_impair.argtypes)[:4] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]


def test_constants_and_an_unchanged_abi_version():
    from wifirx import capi
    raw = _header_raw()
    for name, value in (("WIFIRX_FE_DC", "1u"), ("WIFIRX_FE_IQ", "2u"), ("WIFIRX_FE_BLOCK", "4096"), ("WIFIRX_FE_RING", "64")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), raw), name
    assert (capi.FE_DC, capi.FE_IQ, capi.FE_BLOCK, capi.FE_RING) == (1, 2, 4096, 64) == (fr.FE_DC, fr.FE_IQ, fr.BLOCK, fr.RING)
    assert re.search(r"#define\s+WIFIRX_ABI_VERSION\s+4\b", raw)               # the additions are additive
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    assert "wifirx_push_diversity returns WIFIRX_EINVAL" in raw and "wifirx_channelize has no" in raw     # the header says what is out of scope


def test_struct_layouts_against_a_c_compiler():
    from wifirx import capi
    fields = ["n", "part", "ring", "d0", "w0"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "wifirx.h"\nint main(void){printf("%zu %zu", sizeof(wifirx_frontend_cfg), '
           'sizeof(wifirx_frontend_state));\n' +
           "".join('printf(" %%zu", offsetof(wifirx_frontend_state, %s));\n' % f for f in fields) +
           "".join('printf(" %%zu", offsetof(wifirx_frontend_cfg, %s));\n' % f for f in ("flags", "frac_bits", "dc_shift", "iq_shift")) +
           'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o",
                               os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert got[:2] == [C.sizeof(capi.FrontendCfg), capi.FE_STATE_DTYPE.itemsize] == [16, 2632]
    assert got[2:7] == [capi.FE_STATE_DTYPE.fields[f][1] for f in fields] == [0, 8, 48, 2608, 2624]
    assert got[7:] == [getattr(capi.FrontendCfg, f).offset for f in ("flags", "frac_bits", "dc_shift", "iq_shift")] == [0, 4, 8, 12]
    assert capi.FE_STATE_DTYPE == fr.STATE_DTYPE


def test_estimate_on_the_host_equals_the_restatement():
    """wifirx_frontend_estimate needs no device: the states of a restated stream, cut at several lengths"""
    from wifirx import capi
    rng = np.random.default_rng(11)
    x = ((rng.standard_normal(21 * 4096) + 1j * rng.standard_normal(21 * 4096)) * 0.7).astype(np.complex64)
    x = fr.rx_impair(x, *fr.imbalance(1.0, 5.0), 0.3 - 0.6j)
    init = capi.frontend_state(d0=0.25 - 0.125j, w0=0.03 + 0.01j)
    for flags, (dc, iq) in ((0, (False, False)), (1, (True, False)), (2, (False, True)), (3, (True, True))):
        for n in (0, 100, 4096, 4097, 3 * 4096 + 17, 17 * 4096, 21 * 4096):
            for shifts in ((2, 4), (0, 6), (6, 0)):
                fe = fr.Frontend(flags=flags, dc_shift=shifts[0], iq_shift=shifts[1], state=init)
                fe.process(x[:n])
                cfg = capi.frontend_cfg(dc=dc, iq=iq, dc_shift=shifts[0], iq_shift=shifts[1])
                got, want = capi.frontend_estimate(cfg, fe.state()), fe.estimate()
                assert [np.atleast_1d(g).view(np.uint32).tolist() for g in got] == [np.atleast_1d(w).view(np.uint32).tolist() for w in want], (flags, n, shifts)


def test_estimate_refuses_a_bad_cfg():
    from wifirx import capi
    st = np.zeros((), capi.FE_STATE_DTYPE)
    d, w = (C.c_float * 2)(), (C.c_float * 2)()
    lib = capi.lib()
    for bad in (capi.FrontendCfg(4, 12, 2, 4), capi.FrontendCfg(1, 31, 2, 4), capi.FrontendCfg(1, 12, 7, 4), capi.FrontendCfg(1, 12, 2, 7)):
        assert lib.wifirx_frontend_estimate(C.byref(bad), st.ctypes.data_as(C.c_void_p), d, w) == capi.EINVAL
    good = capi.frontend_cfg()
    assert lib.wifirx_frontend_estimate(None, st.ctypes.data_as(C.c_void_p), d, w) == capi.EINVAL
    assert lib.wifirx_frontend_estimate(C.byref(good), None, d, w) == capi.EINVAL
    assert lib.wifirx_frontend_estimate(C.byref(good), st.ctypes.data_as(C.c_void_p), None, w) == capi.EINVAL
    assert lib.wifirx_frontend_estimate(C.byref(good), st.ctypes.data_as(C.c_void_p), d, w) == capi.OK


def test_python_surface():
    from wifirx import block, capi
    for name in ("frontend_dev", "frontend", "rx_impair_dev", "rx_impair", "stream_frontend", "stream_frontend_state"):
        assert callable(getattr(capi.WifiRx, name)), name
    cfg = capi.frontend_cfg()
    assert (cfg.flags, cfg.frac_bits, cfg.dc_shift, cfg.iq_shift) == (capi.FE_DC, 12, 2, 4)        # rule 32's defaults: IQ off
    assert capi.frontend_cfg(dc=False, iq=True).flags == capi.FE_IQ
    assert capi.iq_imbalance() == (1 + 0j, 0j) and capi.iq_imbalance(1.0, 5.0) == fr.imbalance(1.0, 5.0)
    prm = inspect.signature(block.wifi_phy_rx.__init__).parameters
    assert [prm[k].default for k in ("dc_block", "iq_correct", "fe_frac_bits", "fe_dc_shift", "fe_iq_shift")] == [False, False, 12, 2, 4]
    for name in ("set_dc_block", "set_iq_correct"):
        assert callable(getattr(block.wifi_phy_rx, name)), name
    prm = inspect.signature(block.channel_model.__init__).parameters
    assert [prm[k].default for k in ("dc_offset", "iq_gain_db", "iq_phase_deg")] == [0j, 0.0, 0.0]
