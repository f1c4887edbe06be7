"""CPU test of the bilinear tap the flow post-processing kernels share (denseflow_amd/csrc/flow_quad.h: fq_tap, fq_lerp and the
samplers built on them).

The header that is compiled into the HIP kernels is compiled here with g++ -ffp-contract=off into tests/flow_quad_harness.cpp,
which prints the tap geometry and the samples of probe images for a list of positions.  They are held bit for bit against the
NumPy references the kernels themselves are tested with, not against a restatement: position (px, py) is the flow of pixel
(0, 0) of an otherwise zero flow, so tests/warp_ref.py gives `inside` and the samples of the 8-bit probe under both borders,
and tests/fb_check_ref.py gives `inside` and, from the samples of the two float probe planes, err.  Two channels of the 8-bit
probe are ramps (the column and the row index), so the reference's samples of them are x0 + ax and y0 + ay and pin the
harness's floor and frac of either axis directly; x1 and y1 are the neighbour, or the last column and row themselves.  The range test before the
cast is pinned on the very function the kernels compile, and the harness runs once more under
-fsanitize=undefined,address, where a float out of int's range reaching a cast, or a tap outside its image, ends the run."""
import os
import subprocess

import numpy as np
import pytest

from tests import fb_check_ref, warp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
SIZES = [(1, 1), (2, 1), (1, 2), (5, 3)]
BORDERS = {"zero": 0, "clamp": 1}  # FQ_BORDER_* of the header


def _axis(n):
    """The coordinates asked of an axis of n pixels: every integer, n - 1 exactly (among them) and one ulp either side, -0.0,
    the largest negative subnormal, both infinities, NaN, +-1e30."""
    last = F32(n - 1)
    vals = [F32(i) for i in range(n)] + [np.nextafter(last, F32(-np.inf)), np.nextafter(last, F32(np.inf)), F32(-0.0),
                                         -np.nextafter(F32(0), F32(1)), F32(np.inf), F32(-np.inf), F32(np.nan), F32(1e30),
                                         F32(-1e30)]
    return np.array(vals, F32)


def _positions(w, h):
    xs, ys = _axis(w), _axis(h)
    return np.array([(x, y) for y in ys for x in xs], F32)


def _probes(w, h):
    rng = np.random.default_rng(100 * w + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # channel 0 is the column index and channel 1 the row index: their samples are x0 + ax * (x1 - x0) and y0 + ay * (y1 - y0),
    # exactly (the other axis lerps between equal values), so the reference's samples pin floor and frac of either axis
    img[..., 0], img[..., 1] = np.arange(w)[None, :], np.arange(h)[:, None]
    planes = rng.uniform(-3, 3, (2, h, w)).astype(F32)
    if w * h >= 15:  # the lerp is never shortcut: a tap of inf or NaN shows, with a weight of 0 too
        planes[0, 1, 2], planes[1, 2, 3], planes[0, 2, 4] = np.inf, np.nan, -np.inf
    return img, planes


def _hex(a):
    return " ".join("%08x" % v for v in np.asarray(a, F32).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def harnesses():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    built = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=undefined,address",
                                                           "-fno-sanitize-recover=all"])):
        exe = os.path.join(out_dir, "flow_quad_harness_%s.%d" % (name, os.getpid()))
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
            "-o", exe, os.path.join(HERE, "flow_quad_harness.cpp")]
        subprocess.run(cmd, check=True, capture_output=True)
        built[name] = exe
    yield built
    for exe in built.values():
        os.unlink(exe)


def _run(exe, w, h, border, img, planes, pos):
    text = "%d %d %d\n%s\n%s\n" % (w, h, BORDERS[border], " ".join(str(int(v)) for v in img.reshape(-1)), _hex(planes))
    text += "".join("%s\n" % _hex(p) for p in pos)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [line.replace("|", " ").split() for line in r.stdout.splitlines()]
    assert len(rows) == len(pos)
    geo = np.array([[int(v) for v in row[:6]] for row in rows], np.int64)
    flt = np.array([[int(v, 16) for v in row[6:]] for row in rows], np.uint32).view(F32)
    return geo, flt


def _same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("border", list(BORDERS))
@pytest.mark.parametrize("w,h", SIZES)
def test_tap_and_lerp_are_the_references_bit_for_bit(harnesses, w, h, border):
    img, planes = _probes(w, h)
    pos = _positions(w, h)
    geo, flt = _run(harnesses["plain"], w, h, border, img, planes, pos)
    for (px, py), (inside, take, x0, x1, y0, y1), f in zip(pos, geo, flt):
        ax, ay, gray, il, pl, su, sv = f[0], f[1], f[2], f[3:6], f[6:9], f[9], f[10]
        flow = np.zeros((2, h, w), F32)
        flow[0, 0, 0], flow[1, 0, 0] = px, py  # pixel (0, 0): the position is the flow itself (-0.0 arrives as +0.0)
        where = "w %d h %d %s px %r py %r" % (w, h, border, px, py)
        s, valid = warp_ref.warp(img, flow, border)
        assert inside == int(warp_ref.inside_of(flow)[0, 0]) == int(valid[0, 0]), where
        assert inside == int(not fb_check_ref.out_of_frame(flow)[0, 0]), where
        assert _same_bits(il, s[0, 0]) and _same_bits(pl, s[0, 0]) and _same_bits(gray, s[0, 0, 0]), where
        # the taps lie in the image whatever the position was; one that is not taken is (0, 0) and samples nothing
        assert 0 <= x0 <= x1 <= w - 1 and 0 <= y0 <= y1 <= h - 1 and 0 <= ax < 1 and 0 <= ay < 1, where
        if not take:
            assert not inside and (x0, y0, ax, ay) == (0, 0, 0, 0) and not s[0, 0].any(), where
        else:  # floor and frac of either axis, through the reference's samples of the two ramps
            assert _same_bits(F32(x0) + ax * F32(x1 - x0), s[0, 0, 0]) and _same_bits(F32(y0) + ay * F32(y1 - y0), s[0, 0, 1]), where
            assert x1 - x0 == (1 if x0 < w - 1 else 0) and y1 - y0 == (1 if y0 < h - 1 else 0), where
        if border == "zero":  # the forward-backward check samples the float planes at the same tap
            assert take == inside, where
            occ, err = fb_check_ref.fb_check(flow, planes)
            if inside:
                with np.errstate(all="ignore"):
                    du, dv = F32(flow[0, 0, 0]) + su, F32(flow[1, 0, 0]) + sv
                    want = du * du + dv * dv
                assert _same_bits(err[0, 0], want), where
            else:
                assert occ[0, 0] == 1 and np.isposinf(err[0, 0]), where


@pytest.mark.parametrize("border", list(BORDERS))
@pytest.mark.parametrize("w,h", SIZES)
def test_no_cast_and_no_tap_trips_a_sanitizer(harnesses, w, h, border):
    img, planes = _probes(w, h)
    pos = _positions(w, h)
    geo, flt = _run(harnesses["plain"], w, h, border, img, planes, pos)
    geo_s, flt_s = _run(harnesses["sanitized"], w, h, border, img, planes, pos)
    assert np.array_equal(geo, geo_s) and _same_bits(flt, flt_s)
