"""wifirx_irs_taps_multi and wifirx_irs_sweep_multi in the C ABI and the Python surface: the declarations word for word, the ctypes
prototypes, the ABI version, the header comments, and the constructor checks of IrsConfig(antennas=) and channel_model, all on a
box without a GPU.  (The host checks of the entry points need a handle: tests/test_gpu_irs_multi.py.)"""
import inspect
import re

import numpy as np
import pytest

from abi_helpers import _decl, _header, _header_raw, _norm

SCENE = ["wifirx_handle* h", "float* taps_out", "uint32_t n_ant", "uint32_t n_sets", "uint32_t n_taps", "const float* pdp", "float gain",
         "uint32_t n_elems", "const float* los_b2r", "const float* los_r2u", "const float* los_b2u", "float k_factor",
         "float direct_gain"]
TAPS = SCENE + ["const float* psi", "int psi_on_device", "uint32_t n_psi_sets", "uint32_t align_bits", "const float* scatter",
                "uint32_t n_scatter", "uint64_t irs_seed", "float* elems_out", "uint8_t* codes_out"]
SWEEP = SCENE + ["const float* codebook", "int codebook_on_device", "uint32_t n_codes", "const float* scatter", "uint32_t n_scatter",
                 "uint64_t irs_seed", "uint16_t* best_out", "float* power_out"]


def test_symbols_declared_exported_and_listed():
    from wifirx import capi
    for name in ("wifirx_irs_taps_multi", "wifirx_irs_sweep_multi"):
        assert re.search(r"\bint\s+%s\s*\(" % name, _header())
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert capi.lib().wifirx_abi_version() == capi.ABI_VERSION == 4          # additive: the version stays


@pytest.mark.parametrize("name,want", [("wifirx_irs_taps_multi", TAPS), ("wifirx_irs_sweep_multi", SWEEP)])
def test_arguments_word_for_word(name, want):
    import ctypes as C
    from wifirx import capi
    assert _norm(_decl(_header(), name)) == want
    kinds = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}
    types = [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in want]
    assert list(getattr(capi.lib(), name).argtypes) == types
    # the single-antenna call with n_ant behind taps_out
    old = _norm(_decl(_header(), name[:-len("_multi")]))
    assert want[:2] + want[3:] == old and want[2] == "uint32_t n_ant"


def test_header_comments_carry_the_rules():
    raw = _header_raw()
    at = raw.index("int  wifirx_irs_taps_multi(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for word in ("NUMERICS.md rule 27", "b_n       = mix(B_n, w_b(n,r,l))                      shared by all antennas",
                 "a_{m,n}   = mix(A_{m,n}, w_a(m,n,r,l))", "h_{d,m}   = direct_gain * mix(D_m, w_d(m,r,l))",
                 "t_{m,r,l} = s_l (h_{d,m} + sum_n (a_{m,n} psi_n) b_n)", "1 <= M <= 8", "[n_ant][n_sets][n_taps]", "antenna-major",
                 "the genie of the reference antenna", "ANTENNA 0, TAP 0", "(n, r, l + 16 ((m + 1) >> 1), 2)",
                 "(0xFFFFFFFF, r,", "when m is odd", "when m is even", "[n_scatter][(M + 1) N + M]", "(r L + l) % n_scatter",
                 "[n_sets][n_taps][n_ant + 1][N]", "n_ant outside 1..8", "WIFIRX_EINVAL", "WIFIRX_ERANGE", "ORDER: as wifirx_channel"):
        assert word in comment, word
    at = raw.index("int  wifirx_irs_sweep_multi(")
    comment = raw[raw.rindex("/*", 0, at):at]
    for word in ("NUMERICS.md rule 28", "e_{m,n} = ch_mul(a_{m,n}, b_n)", "rho = m L + l", "multiple of 4", "v_mfma_f32_16x16x4_f32",
                 "VALU fmaf chain", "t_{m,l,k}   = s_l (h_{d,m} + y)", "q = re re + im im, without fma",
                 "P_{r,k}     = q_0 + q_1 + ... + q_{ML-1}", "ascending rho", "starting from q_0", "MRC receiver", "equal noise per antenna",
                 "strict >", "lowest k wins a tie", "NaN never wins", "Per-antenna noise weights and selection-combining metrics are not",
                 "At n_ant = 1 this is wifirx_irs_sweep exactly", "n_ant outside 1..8", "ORDER: as wifirx_channel"):
        assert word in comment, word


def test_python_surface():
    from wifirx import block, capi, irs
    for name in ("irs_taps_multi_dev", "irs_taps_multi", "irs_sweep_multi_dev", "irs_sweep_multi"):
        assert callable(getattr(capi.WifiRx, name))
    prm = inspect.signature(capi.WifiRx.irs_taps_multi_dev).parameters
    assert list(prm)[:7] == ["self", "taps_ptr", "n_sets", "pdp", "los_b2r", "los_r2u", "los_b2u"] and prm["los_b2u"].default is None
    assert prm["k_factor"].default == 0.0 and prm["direct_gain"].default == 1.0 and prm["gain"].default == 1.0
    assert prm["align_bits"].default == 0 and prm["scatter"].default is None and prm["seed"].default == 0
    assert prm["elems_ptr"].default is None and prm["codes_ptr"].default is None
    prm = inspect.signature(capi.WifiRx.irs_sweep_multi_dev).parameters
    assert prm["codebook"].kind is inspect.Parameter.KEYWORD_ONLY and prm["codebook"].default is inspect.Parameter.empty
    assert prm["best_ptr"].default is None and prm["power_ptr"].default is None
    assert capi.IRS_MAX_ANT == 8
    sig = inspect.signature(irs.los).parameters
    assert list(sig) == ["irs_scale", "irs_pos", "ap_pos", "user_pos", "antennas"] and sig["antennas"].default is None
    assert "antennas" in inspect.signature(irs.IrsConfig).parameters and irs.IrsConfig.__dataclass_fields__["antennas"].default == 1
    assert isinstance(block.channel_model.irs_best, property)


def test_config_checks():
    from wifirx import irs
    geo = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))
    one = irs.IrsConfig(**geo, psi=np.ones(16))
    assert one.antennas == 1 and one.los_b2r.shape == (16,) and one.los_b2u == complex(1.0)       # the default is what it was
    c = irs.IrsConfig(**geo, psi=np.ones(16), antennas=4)
    assert c.antennas == 4 and c.n_elems == 16 and c.los_b2r.shape == (4, 16) and c.los_b2r.dtype == np.complex64
    assert c.los_b2r.flags.c_contiguous and c.los_r2u.shape == (16,) and c.los_b2u.shape == (4,) and c.los_b2u.dtype == np.complex64
    want = irs.los(4, geo["irs_pos"], geo["ap_pos"], geo["user_pos"], antennas=4)
    assert np.array_equal(c.los_b2r, want[0].astype(np.complex64)) and np.array_equal(c.los_b2u, want[2].astype(np.complex64))
    assert np.array_equal(c.los_b2r[0], one.los_b2r)
    cb = irs.dft_codebook(4)
    assert irs.IrsConfig(**geo, codebook=cb, antennas=8).codebook.shape == (16, 16)
    assert irs.IrsConfig(**geo, align_bits=2, antennas=2).align_bits == 2
    # the vectors themselves, with the shapes of M antennas
    a, b, d = np.ones((3, 5)), np.ones(5), np.ones(3)
    g = irs.IrsConfig(los_b2r=a, los_r2u=b, los_b2u=d, psi=np.ones(5), antennas=3)
    assert g.los_b2r.shape == (3, 5) and g.n_elems == 5
    assert irs.IrsConfig(los_b2r=a, los_r2u=b, direct_gain=0.0, psi=np.ones(5), antennas=3).los_b2u is None
    bad = [dict(geo, psi=np.ones(16), antennas=0), dict(geo, psi=np.ones(16), antennas=9),
           dict(los_b2r=a, los_r2u=b, los_b2u=d, psi=np.ones(5), antennas=2),               # 3 rows for 2 antennas
           dict(los_b2r=np.ones(5), los_r2u=b, los_b2u=d, psi=np.ones(5), antennas=3),       # one row for 3 antennas
           dict(los_b2r=a, los_r2u=np.ones(4), los_b2u=d, psi=np.ones(5), antennas=3),
           dict(los_b2r=a, los_r2u=b, los_b2u=np.ones(2), psi=np.ones(5), antennas=3),
           dict(los_b2r=a, los_r2u=b, psi=np.ones(5), antennas=3),                           # a direct path needs los_b2u
           dict(los_b2r=a, los_r2u=b, los_b2u=d, psi=np.ones(4), antennas=3),
           dict(los_b2r=a, los_r2u=b, los_b2u=d, codebook=np.ones((4, 4)), antennas=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            irs.IrsConfig(**kw)


def test_block_constructor_checks():
    """the constructor refuses before it needs a device: the port count is IrsConfig's, taps and doppler stay excluded"""
    from wifirx import block, irs
    geo = dict(scale=4, irs_pos=(0.015, 0.015, 0), ap_pos=(0.06, 0.06, 4.5), user_pos=(0.36, -0.14, 1.0))
    c = irs.IrsConfig(**geo, psi=np.ones(16), antennas=2)
    with pytest.raises(ValueError):
        block.channel_model(irs=c, taps=(1.0, 0.5))
    with pytest.raises(ValueError):
        block.channel_model(irs=c, doppler=1e-4)
    with pytest.raises(TypeError):
        block.channel_model(irs=dict(antennas=2))
