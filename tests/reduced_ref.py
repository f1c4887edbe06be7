"""NumPy restatement of the one conversion a typed planar store applies to the float32 value it would otherwise store
(dfx_calc_batch_planar_as*, include/dfx.h): round to nearest, ties to even.

float16 is numpy's own astype (IEEE binary16: subnormals produced, +-inf from 65520 on, signed zeros kept).  numpy has no
bfloat16, so that one is the integer rule on the float32 bits and comes back as uint16 bit patterns.  Checked against
torch's CPU conversions in tests/test_reduced_ref.py."""
import numpy as np

BF16_NAN = np.uint16(0x7FC0)


def to_f16_bits(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return x.astype(np.float16).view(np.uint16)


def to_bf16_bits(x) -> np.ndarray:
    """(bits + 0x7FFF + ((bits >> 16) & 1)) >> 16 on the float32 bits; a NaN stays a NaN (its payload is unspecified: one
    quiet pattern here, compare NaN-ness with is_nan_bits)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bits = x.view(np.uint32).astype(np.uint64)
    out = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(x)] = BF16_NAN
    return out


def reduce_bits(x, dtype) -> np.ndarray:
    """uint16 bit patterns of x in "float16" / "bfloat16"."""
    if dtype == "float16":
        return to_f16_bits(x)
    if dtype == "bfloat16":
        return to_bf16_bits(x)
    raise ValueError(dtype)


def is_nan_bits(bits, dtype) -> np.ndarray:
    bits = np.asarray(bits, dtype=np.uint16)
    if dtype == "float16":
        return (bits & 0x7FFF) > 0x7C00
    return (bits & 0x7FFF) > 0x7F80


def bf16_bits_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def special_values() -> np.ndarray:
    """The operands on which a conversion can go wrong: signed zeros, ties, half subnormals, the float16 overflow
    threshold, bfloat16 carries into the exponent, a float32 subnormal."""
    f = np.float32
    vals = [0.0, -0.0,
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),  # float16 ties
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),      # bfloat16 ties
            2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25,             # half subnormals
            -(2.0 ** -24), -(2.0 ** -25),
            65504.0, 65519.996, 65520.0, 3.4e38, -65504.0, -65519.996, -65520.0, -3.4e38,
            1e-40, -1e-40]
    x = np.array(vals, dtype=f)
    carries = np.array([0x3F7FFFFF, 0x7F7FFFFF, 0xBF7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(f)  # to +-1.0, to +-inf
    return np.concatenate([x, carries])
