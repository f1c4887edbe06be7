"""CPU test of the helpers denseflow_amd/csrc/flow_quad.h gained for the warp of typed planes (fq_nearest, the exact half to
float conversions, the typed tap load and sample).

The header that is compiled into the HIP kernels is compiled here with g++ -ffp-contract=off into
tests/plane_warp_harness.cpp, exactly as tests/test_flow_quad_cpu.py compiles its harness, and held bit for bit against
tests/plane_warp_ref.py on a million random bit patterns of positions, on the edge positions of every axis, and over all 65536
patterns of each half type.  The harness runs once more under -fsanitize=undefined,address, where a float out of int's range
reaching a cast, or a tap outside its plane, ends the run.  (On the device fq_f16_to_f32 is the compiler's conversion
instruction; tests/test_plane_warp_gpu.py holds that one to the same reference.)"""
import os
import subprocess

import numpy as np
import pytest

from tests import plane_warp_ref as R
from tests.test_flow_quad_cpu import _axis

HERE = os.path.dirname(os.path.abspath(__file__))
F32, U32, I32 = np.float32, np.uint32, np.int32
ELEM = {"float32": 0, "float16": 1, "bfloat16": 2}  # DFX_ELEM_* of the headers


@pytest.fixture(scope="module")
def harnesses():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    built = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=undefined,address",
                                                           "-fno-sanitize-recover=all"])):
        exe = os.path.join(out_dir, "plane_warp_harness_%s.%d" % (name, os.getpid()))
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
            "-o", exe, os.path.join(HERE, "plane_warp_harness.cpp")]
        subprocess.run(cmd, check=True, capture_output=True)
        built[name] = exe
    yield built
    for exe in built.values():
        os.unlink(exe)


def _run(exe, mode, data=b""):
    r = subprocess.run([exe, mode], input=data, capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _positions(rng, w, h, count):
    """count positions: random bit patterns, random positions round the image, and every pair of the axes' edge values."""
    bits = rng.integers(0, 2 ** 32, (count // 2, 2), dtype=np.uint64).astype(U32).view(F32)
    near = (rng.uniform(-2, 2, (count - count // 2, 2)) * [w, h]).astype(F32)
    half = np.array([(x + d, y + e) for x in range(w) for y in range(h) for d in (0.5, -0.5) for e in (0.5, 0.0)], F32)  # the ties
    edges = np.array([(x, y) for y in _axis(h) for x in _axis(w)], F32)
    return np.ascontiguousarray(np.concatenate([bits, near, half, edges]))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_half_conversions_over_all_65536_patterns(harnesses, build):
    got = np.frombuffer(_run(harnesses[build], "half"), U32).reshape(2, 65536)
    every = np.arange(65536, dtype=U32).astype(np.uint16)
    for row, dtype in ((0, "float16"), (1, "bfloat16")):
        want = R.to_f32(every, dtype)
        assert np.array_equal(got[row], want.view(U32)), dtype  # NaN payloads included


@pytest.mark.parametrize("build,count", [("plain", 1000000), ("sanitized", 100000)])
@pytest.mark.parametrize("border", R.BORDERS)
def test_nearest_positions(harnesses, build, count, border):
    for w, h in ((5, 3), (1, 1), (640, 360)):
        pos = _positions(np.random.default_rng(w), w, h, count // 3)
        head = np.array([w, h, R.BORDERS.index(border), len(pos)], I32)
        got = np.frombuffer(_run(harnesses[build], "nearest", head.tobytes() + pos.tobytes()), I32).reshape(-1, 4)
        inside, take, px, py = R.take_of(pos[:, 0], pos[:, 1], w, h, border)
        xn, yn = R.nearest_at(px, py)
        assert np.array_equal(got[:, 0] != 0, inside) and np.array_equal(got[:, 1] != 0, take)
        assert np.array_equal(got[:, 2], xn) and np.array_equal(got[:, 3], yn)
        assert xn.min() >= 0 and xn.max() <= w - 1 and yn.min() >= 0 and yn.max() <= h - 1  # always in range


@pytest.mark.parametrize("build,count", [("plain", 1000000), ("sanitized", 100000)])
@pytest.mark.parametrize("dtype", R.FLOATS)
def test_typed_samples(harnesses, build, count, dtype):
    w, h = 37, 23
    rng = np.random.default_rng(ELEM[dtype])
    for border in R.BORDERS:
        v = rng.standard_normal((h, w)).astype(F32) * F32(100)
        v[1, 2], v[2, 3], v[2, 4], v[5, 5] = np.inf, np.nan, -np.inf, -0.0
        plane = v if dtype == "float32" else R.stored(v, dtype)
        if dtype != "float32":  # a few random patterns: subnormals, NaN payloads
            plane[rng.random(plane.shape) < 0.02] = rng.integers(0, 65536)
        pos = _positions(rng, w, h, count // 2)
        head = np.array([w, h, R.BORDERS.index(border), ELEM[dtype], len(pos)], I32)
        got = np.frombuffer(_run(harnesses[build], "sample", head.tobytes() + plane.tobytes() + pos.tobytes()), F32)
        _, take, px, py = R.take_of(pos[:, 0], pos[:, 1], w, h, border)
        want = np.where(take, R.bilinear_at(R.to_f32(plane, dtype)[..., None], px, py)[..., 0], F32(0))
        assert R.same(got, want.astype(F32), "float32")
        assert take.sum() > len(pos) // 40  # 1 / 16 of the positions round the image lie inside it
