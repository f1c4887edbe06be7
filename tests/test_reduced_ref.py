"""tests/reduced_ref.py — the NumPy restatement of the float16 / bfloat16 conversion of the typed planar output — against
torch's CPU conversions, on random values and on the special operands."""
import numpy as np
import pytest

from tests import reduced_ref as R


def _operands():
    rng = np.random.default_rng(3)
    rand = (rng.standard_normal(4096) * 8).astype(np.float32)
    wide = rng.integers(0, 2 ** 32, 8192, dtype=np.uint64).astype(np.uint32).view(np.float32)  # every exponent, NaNs too
    return np.concatenate([R.special_values(), rand, wide, np.array([np.nan, -np.nan, np.inf, -np.inf], np.float32)])


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_restatement_is_torchs_cpu_conversion(dtype):
    import torch

    x = _operands()
    tdt = torch.float16 if dtype == "float16" else torch.bfloat16
    want = torch.from_numpy(x.copy()).to(tdt).view(torch.int16).numpy().view(np.uint16)
    got = R.reduce_bits(x, dtype)
    nan = np.isnan(x)
    assert got.dtype == np.uint16 and got.shape == x.shape
    assert R.is_nan_bits(got[nan], dtype).all() and R.is_nan_bits(want[nan], dtype).all()
    assert not R.is_nan_bits(got[~nan], dtype).any()
    bad = np.flatnonzero(got[~nan] != want[~nan])
    assert bad.size == 0, (x[~nan][bad[:8]], got[~nan][bad[:8]], want[~nan][bad[:8]])


def test_the_named_special_cases():
    f16 = lambda v: int(R.to_f16_bits(np.array([v], np.float32))[0])  # noqa: E731
    bf = lambda v: int(R.to_bf16_bits(np.array([v], np.float32))[0])  # noqa: E731
    assert f16(0.0) == 0x0000 and f16(-0.0) == 0x8000 and bf(-0.0) == 0x8000
    assert f16(1 + 2.0 ** -11) == 0x3C00 and f16(1 + 3 * 2.0 ** -11) == 0x3C02  # ties go to the even neighbour
    assert bf(1 + 2.0 ** -8) == 0x3F80 and bf(1 + 3 * 2.0 ** -8) == 0x3F82
    assert f16(2.0 ** -24) == 0x0001 and f16(1.5 * 2.0 ** -24) == 0x0002 and f16(2.0 ** -25) == 0x0000  # subnormals kept
    assert f16(2.0 ** -14 - 2.0 ** -25) == 0x0400  # rounds up into the smallest normal
    assert f16(65504.0) == 0x7BFF and f16(65519.996) == 0x7BFF and f16(65520.0) == 0x7C00 and f16(-3.4e38) == 0xFC00
    x = np.array([0x3F7FFFFF, 0x7F7FFFFF], np.uint32).view(np.float32)
    assert list(R.to_bf16_bits(x)) == [0x3F80, 0x7F80]  # the carry runs into the exponent: 1.0, inf
    assert bf(1e-40) == 0x0001 and f16(1e-40) == 0x0000
    assert R.is_nan_bits(R.to_bf16_bits(np.array([np.nan], np.float32)), "bfloat16").all()
