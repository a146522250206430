"""wifirx_channel_sro and wifirx_resampler_table in the C ABI, on a box without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported_and_declared():
    from wifirx import capi
    txt = open(os.path.join(ROOT, "include", "wifirx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in ("wifirx_channel_sro", "wifirx_resampler_table"):
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), s
        assert s in capi.EXPORTS and hasattr(capi.lib(), s), s
    # additive: the version stays, and wifirx_channel keeps its 17 arguments
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4
    decl = re.search(r"\bwifirx_channel_sro\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    assert re.search(r"const\s+float\s*\*\s*sro\s*,\s*int64_t\s+drift0", decl)
    assert len(decl.split(",")) == 19 and len(capi.lib().wifirx_channel_sro.argtypes) == 19
    assert len(capi.lib().wifirx_channel.argtypes) == 17


def test_table_getter_needs_no_device():
    from wifirx import capi
    lib = capi.lib()
    p, n_ph, n_t = C.POINTER(C.c_float)(), C.c_uint32(), C.c_uint32()
    assert lib.wifirx_resampler_table(C.byref(p), C.byref(n_ph), C.byref(n_t)) == capi.OK
    assert (n_ph.value, n_t.value) == (128, 32) and bool(p)
    assert lib.wifirx_resampler_table(None, None, None) == capi.OK
    q = C.POINTER(C.c_float)()
    assert lib.wifirx_resampler_table(C.byref(q), None, None) == capi.OK
    assert C.addressof(q.contents) == C.addressof(p.contents), "the table is one object owned by the library"
    T = capi.resampler_table()
    assert T.shape == (129, 32) and T[0, 15] == 1.0 and T[128, 16] == 1.0


def test_committed_header_is_the_generator_output():
    """csrc/wr_resample_table.h is what tools/gen_resample_table.py writes, and the library's table is its float32 design"""
    import importlib.util
    from wifirx import capi
    spec = importlib.util.spec_from_file_location("gen_resample_table", os.path.join(ROOT, "tools", "gen_resample_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    T = gen.design()
    # the linear algebra may differ in the last bits between LAPACK builds: the committed table is the design to 1e-6
    assert np.abs(capi.resampler_table().astype(np.float64) - T.astype(np.float64)).max() <= 1e-6
    assert gen.render(capi.resampler_table()) == open(gen.HEADER).read()


def test_drift_inc_matches_its_definition():
    from wifirx import capi
    import resample_ref
    assert capi.drift_inc(0.0) == 0
    assert capi.drift_inc(2.0 ** -8) == 1 << 32 and capi.drift_inc(-2.0 ** -8) == -(1 << 32)
    assert capi.drift_inc(2.0 ** -41) == 1 and capi.drift_inc(-2.0 ** -41) == -1       # halves round away from zero
    assert capi.drift_inc(2.0 ** -42) == 0
    assert capi.drift_inc(-20e-6) == -capi.drift_inc(20e-6) == -round(float(np.float32(20e-6)) * 2 ** 40)
    rng = np.random.default_rng(0)
    for s in np.concatenate([rng.uniform(-2.0 ** -8, 2.0 ** -8, 200), rng.uniform(-1e-9, 1e-9, 50)]).astype(np.float32):
        want = resample_ref.drift_inc(s)                       # exact integer arithmetic
        assert capi.drift_inc(s) == want, s
        assert abs(want - float(s) * 2.0 ** 40) <= 0.5


def test_python_keywords():
    from wifirx import capi
    for f in (capi.WifiRx.channel, capi.WifiRx.channel_dev):
        prm = inspect.signature(f).parameters
        assert prm["sro"].default is None and prm["drift0"].default == 0
    cfo = np.float32(0.037)
    assert abs(float(capi.locked_sro(cfo)) + 20e-6) < 1e-8     # +20 ppm of 5.89 GHz at 20 MS/s -> epsilon - 1 = -20 ppm
