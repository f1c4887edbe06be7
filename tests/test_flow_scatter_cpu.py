"""CPU test of the integer scatter the flow projection and the splat share (denseflow_amd/csrc/flow_scatter.h: the landing
rule, the taps, the adds, the LDS window's origin, in-window test and flush).

The header that is compiled into the HIP kernels is compiled here with g++ -ffp-contract=off into
tests/flow_scatter_harness.cpp, which runs the scatter serially, tile after tile in the kernels' order, once with every tap
going straight to the workspace and once through a window array, and prints the workspace words of both.  Both are held word
for word, wrapped sums included, against the sums of the NumPy references the kernels themselves are tested with:
tests/flow_project_ref.sums for three words with the projection's quantisation of the flow, tests/splat_ref.sums for a float
payload of one and of four channels.  The harness runs once more under -fsanitize=undefined,address (and
float-cast-overflow, which GCC leaves out of `undefined`), where a float out of int's range reaching a cast, or a window or
workspace index out of bounds, ends the run."""
import os
import subprocess

import numpy as np
import pytest

from tests import flow_project_ref as P
from tests import splat_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
F32, U32, U64 = np.float32, np.uint32, np.uint64
SHAPES = [(1, 1), (3, 2), (5, 1), (13, 9), (33, 9), (97, 61)]  # (33, 9): one full tile, a ragged second column and row of tiles
TS = [1.0, 0.5, -1.0]
TW, TH = 32, 8  # the source tile of a workgroup (FS_TW, FS_TH of the header)
# tests/test_flow_project_gpu.py, test_special_importances
IMPORTANCES = np.array([np.nan, 0.0, -0.0, -1.0, 1e-3, 1.0 / 512, 1.0 / 513, 256.0, 257.0, 1e9, np.inf, -np.inf, 1e-40], F32)


def _plant(flow, i):
    """tests/test_flow_project_gpu.py's _plant for flow i of a batch: landings and values at the edges of the arithmetic,
    planted into flow (2, h, w) in place.  Row-major pixel 5 k + i + 1 (modulo w * h) takes special value k in plane i % 2;
    the landings (exactly -1, one ulp inside it, exactly W or H, one ulp inside it, 0, the last column or row, a half) start
    from column 0 or row 0."""
    _, h, w = flow.shape
    one, c = np.nextafter, i % 2
    for k, v in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0, 1e-40, -1e-40, 1.1754944e-38]):
        flow[c].reshape(-1)[(5 * k + i + 1) % (w * h)] = F32(v)
    edge = w if c == 0 else h
    for k, land in enumerate((-1.0, one(F32(-1), F32(0)), float(edge), one(F32(edge), F32(0)), 0.0, float(edge - 1), 0.5)):
        y, x = ((k + i) % h, 0) if c == 0 else (0, (k + i) % w)
        flow[c, y, x] = F32(land)
        flow[1 - c, y, x] = 0.0
    return flow


def _flows(w, h, t):
    """(name, flow (2, h, w)) of one shape: the GPU tests' smooth flow, their special values and landings in either plane, the
    tile centres NaN or infinite (the window origin takes its bound: every tap goes the global way), and every pixel onto one."""
    base = P.project_inputs(w, h)[0]
    yield "smooth", base[0]
    yield "specials in u", _plant(base[1].copy(), 0)
    yield "specials in v", _plant(base[2].copy(), 1)
    lost = base[0].copy()
    for k, (by, bx) in enumerate((by, bx) for by in range(0, h, TH) for bx in range(0, w, TW)):
        cy, cx = min(by + TH // 2, h - 1), min(bx + TW // 2, w - 1)
        lost[k % 2, cy, cx] = (np.nan, np.inf, -np.inf)[k % 3]
    yield "tile centres not finite", lost
    yy, xx = np.mgrid[0:h, 0:w]
    yield "onto one pixel", (np.stack([w // 2 - xx, h // 3 - yy]) / t).astype(F32)  # exact: t is a power of two


def _hex(a, kind=F32):
    """The bit patterns of a, 8 (float32) or 16 (uint64) hex digits each with nothing between them."""
    a = np.ascontiguousarray(a, kind).reshape(-1)
    return a.view(U32 if kind is F32 else U64).byteswap().tobytes().hex()


def _ints(a):
    return " ".join(map(str, np.asarray(a).astype(np.int64).reshape(-1).tolist()))


@pytest.fixture(scope="module")
def harnesses():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    built = {}
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=undefined,address",
                                                           "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"])):
        exe = os.path.join(out_dir, "flow_scatter_harness_%s.%d" % (name, os.getpid()))
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags + [
            "-o", exe, os.path.join(HERE, "flow_scatter_harness.cpp")]
        subprocess.run(cmd, check=True, capture_output=True)
        built[name] = exe
    yield built
    for exe in built.values():
        os.unlink(exe)


def _case(flow, t, imp, occ, q=None, ok=None):
    """The text of one case of the harness."""
    _, h, w = flow.shape
    text = "%d %d %s %d %d %d\n%s\n" % (w, h, _hex(F32(t)), 0 if q is None else len(q), imp is not None, occ is not None, _hex(flow))
    text += (_hex(imp) if imp is not None else "") + "\n" + (_ints(occ) if occ is not None else "") + "\n"
    if q is not None:
        text += _ints(ok) + "\n" + _ints(q) + "\n"
    return text


def _cases(w, h):
    """(where, text, want (h, w, WORDS) uint64) of every case of one shape: the projection's three words and a float payload
    of one and of four channels, over t, the flows, and no planes, importance and occ, or the special importances."""
    _, imp, occ = P.project_inputs(w, h)
    pay = S.splat_inputs(w, h)[2][0]
    rng = np.random.default_rng(7 * w + h)
    pay[:, rng.random((h, w)) < 0.1] = F32(40000.0)  # a tenth of the payloads is refused
    masks = [("plain", None, None), ("importance and occ", imp[0], occ[0]),
             ("special importances", IMPORTANCES[rng.integers(0, len(IMPORTANCES), (h, w))], None)]
    for t in TS:
        for name, flow in _flows(w, h, t):
            for mask, imp_i, occ_i in masks:
                where = "w %d h %d t %r flow %s, %s" % (w, h, t, name, mask)
                yield where, _case(flow, t, imp_i, occ_i), np.stack([a.view(U64) for a in P.sums(flow, t, imp_i, occ_i)], -1)
                for channels in (1, 4):
                    if name == "onto one pixel":  # the largest payload under the largest importance: the sums wrap at 97 x 61
                        imp_i = None if imp_i is None else np.full((h, w), 300.0, F32)
                        q, ok = S.payload(np.full((channels, h, w), -32768.0, F32))
                    else:
                        q, ok = S.payload(pay[:channels])
                    ws, s = S.sums(q, ok, flow, t, imp_i, occ_i)
                    want = np.concatenate([ws[None].view(np.int64), s]).transpose(1, 2, 0).view(U64)
                    yield "%s, %d channels" % (where, channels), _case(flow, t, imp_i, occ_i, q, ok), want


@pytest.mark.parametrize("w,h", SHAPES)
def test_both_forms_of_the_scatter_give_the_references_words_in_both_builds(harnesses, tmp_path, w, h):
    cases = list(_cases(w, h))
    paths = []
    for k, (_, text, _) in enumerate(cases):
        paths.append(str(tmp_path / ("case%d" % k)))
        with open(paths[-1], "w") as f:
            f.write(text)
    for build in ("plain", "sanitized"):
        r = subprocess.run([harnesses[build]] + paths, capture_output=True, text=True)
        assert r.returncode == 0, (build, r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert len(lines) == 3 * len(cases)
        for k, (where, _, want) in enumerate(cases):
            for form, line in zip(("global", "window"), lines[3 * k:3 * k + 2]):
                assert line == _hex(want, U64), (build, form, where)
            # the window form really adds into its window: every word of the sums went through it where the flow is smooth
            # (no tap is 24 pixels from where its tile's centre lands), none where no tile's centre lands anywhere
            in_window = int(lines[3 * k + 2])
            if "flow smooth" in where:
                assert in_window >= np.count_nonzero(want), (build, where)
                assert np.count_nonzero(want) > 0 or w * h < 13 * 9 or "plain" not in where, (build, where)
            if "tile centres not finite" in where:
                assert in_window == 0, (build, where)


def test_the_inputs_reach_what_they_are_meant_to():
    """At 97 x 61: sums that wrap, a tile centre that is not finite, landings dropped and landings kept among the specials."""
    w, h = 97, 61
    flows = dict(_flows(w, h, 1.0))
    q, ok = S.payload(np.full((1, h, w), -32768.0, F32))
    ws, s = S.sums(q, ok, flows["onto one pixel"], 1.0, np.full((h, w), 300.0, F32), None)
    assert int(ws[h // 3, w // 2]) == w * h << 32 and w * h << 55 >= 1 << 64
    assert int(s[0, h // 3, w // 2]) == (-(w * h << 55) + (1 << 63)) % (1 << 64) - (1 << 63)  # wrapped
    assert not np.isfinite(flows["tile centres not finite"][:, min(TH // 2, h - 1), min(TW // 2, w - 1)]).all()
    ws = P.sums(flows["specials in u"], 1.0)[0]
    assert (ws == 0).any() and (ws > 0).any()

