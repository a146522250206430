"""NumPy reference of the bf16 LLR format (NUMERICS.md rule 15): the IEEE round-to-nearest-even conversion of float32,
NaN to a quiet NaN, +-inf and subnormals kept -- no torch needed (the binding stays torch-free; tests/test_llr_bf16_ref.py
pins this against torch's CPU bfloat16)."""
import numpy as np


def bf16_rne(x) -> np.ndarray:
    """float32 values -> their bf16 bit patterns (np.uint16), round to nearest, ties to even"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    return np.where(nan, ((b >> 16) | 0x0040).astype(np.uint16), r).astype(np.uint16)


def bf16_to_f32(bits) -> np.ndarray:
    """bf16 bit patterns -> float32 (exact)"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def same_bf16(a, b) -> bool:
    """bit-equal, except that any NaN matches any NaN"""
    a, b = np.asarray(a, dtype=np.uint16), np.asarray(b, dtype=np.uint16)
    na, nb = np.isnan(bf16_to_f32(a)), np.isnan(bf16_to_f32(b))
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a[~na], b[~nb]))
