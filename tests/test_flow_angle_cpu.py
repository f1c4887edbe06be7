"""CPU test of the angle the colour coding and the orientation histograms share (denseflow_amd/csrc/flow_angle.h:
fv_atan2_turns, the atan2_turns of include/dfx.h section (0.5.1)).

The header that is compiled into the HIP kernels is compiled here with g++ -ffp-contract=off into tests/flow_angle_harness.cpp,
as tests/test_flow_quad_cpu.py does for flow_quad.h, and held bit for bit against tests/flow_colour_ref.py's atan2_turns — the
NumPy reference the kernels themselves are tested with, not a restatement — on the special arguments (+-0 in every
combination, equal arguments, subnormals, 1e9, the largest finite float) and on more than a million random bit patterns of
finite floats.  The harness runs once more under -fsanitize=undefined."""
import os
import subprocess

import numpy as np
import pytest

from tests.flow_colour_ref import atan2_turns

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


@pytest.fixture(scope="module")
def harnesses():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    built = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out_dir, "flow_angle_harness_%s.%d" % (name, os.getpid()))
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
            "-o", exe, os.path.join(HERE, "flow_angle_harness.cpp")]
        subprocess.run(cmd, check=True, capture_output=True)
        built[name] = exe
    yield built
    for exe in built.values():
        os.unlink(exe)


def _run(exe, y, x):
    pairs = np.stack([np.asarray(y, F32), np.asarray(x, F32)], -1).reshape(-1, 2)
    r = subprocess.run([exe], input=np.ascontiguousarray(pairs).tobytes(), capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.frombuffer(r.stdout, F32)
    assert out.shape == (len(pairs),)
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def _specials():
    tiny, big = np.nextafter(F32(0), F32(1)), np.finfo(F32).max
    vals = [F32(0.0), F32(-0.0), tiny, -tiny, F32(200) * tiny, np.finfo(F32).tiny, F32(1e-30), F32(0.5), F32(-0.5), F32(1.0),
            F32(-1.0), np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0)), F32(3.0), F32(-4.0), F32(1e9), F32(-1e9),
            np.nextafter(F32(1e9), F32(0)), F32(2e9), F32(1e30), big, -big]
    v = np.array(vals, F32)
    return np.repeat(v, len(v)), np.tile(v, len(v))  # every pair, equal arguments among them


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_specials_bit_for_bit(harnesses, build):
    y, x = _specials()
    got, want = _run(harnesses[build], y, x), atan2_turns(y, x)
    assert _same_bits(got, want), [(a, b, g, w) for a, b, g, w in zip(y, x, got, want) if g.tobytes() != w.tobytes()][:5]
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0
    keys = list(zip(y.view(np.uint32).tolist(), x.view(np.uint32).tolist()))  # by bit pattern: -0.0 is not 0.0

    def one(yv, xv):
        return got[keys.index((int(F32(yv).view(np.uint32)), int(F32(xv).view(np.uint32))))]

    # +-0 behave as in IEEE atan2: the sign bits decide
    assert one(0.0, 1.0) == 0 and not np.signbit(one(0.0, 1.0)) and np.signbit(one(-0.0, 1.0))
    assert one(0.0, -1.0) == 1.0 and one(-0.0, -1.0) == -1.0 and one(0.0, -0.0) == 1.0 and one(-0.0, -0.0) == -1.0
    assert abs(one(1.0, 1.0) - 0.25) < 1e-6 and abs(one(1.0, 0.0) - 0.5) < 1e-6 and abs(one(-1.0, -1.0) + 0.75) < 1e-6


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_a_million_random_finite_bit_patterns_bit_for_bit(harnesses, build):
    rng = np.random.default_rng(20)
    count = 1 << 20 if build == "plain" else 1 << 16
    bits = rng.integers(0, 1 << 32, 3 * count, dtype=np.uint64).astype(np.uint32)
    vals = bits.view(F32)
    vals = vals[np.isfinite(vals)][:2 * count]
    assert len(vals) == 2 * count and count >= (1000000 if build == "plain" else 0)
    y, x = vals[:count], vals[count:]
    got, want = _run(harnesses[build], y, x), atan2_turns(y, x)
    assert _same_bits(got, want)
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0
    # the arguments the histograms meet: moderate vectors, where the polynomial is within 1e-6 half-turns of arctan2 / pi
    y, x = (rng.standard_normal((2, count)) * 5).astype(F32)
    got = _run(harnesses[build], y, x)
    assert _same_bits(got, atan2_turns(y, x))
    assert np.abs(got.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)) / np.pi).max() < 1e-6
