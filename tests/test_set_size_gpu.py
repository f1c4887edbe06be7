"""dfx_set_size: a handle re-planned for another frame size inside its allocations computes, bit for bit, what a handle
freshly created at that size with the same params computes — float flows and TVL1 iteration tables, bounded planes, PNG
planes and bounds, JPEG files, colour frames, and the levels / level sizes / batch of dfx_get_stats.

The walk's sizes are the smallest that cross the boundaries a constant W x H was baked into: the 64-float pitch step
(64 / 65 wide), one / two / three 64-column tiles, a TVL1 pyramid that loses levels (20 x 20: the second level would be
16 x 16 — kept — and the third 13 x 13 — dropped; 65 x 33 keeps four of the five), growing (224 x 224 is the only stop
whose pair slots and pyramids exceed what 96 x 64 allocated) and shrinking.  References come from fresh handles, once
per (algorithm, size, params), and are shared by the tests."""
import numpy as np
import pytest

import denseflow_amd
from denseflow_amd import engine as E
from denseflow_amd.synth import ContentClip, SynthClip

pytestmark = pytest.mark.gpu

WALK = [(96, 64), (65, 33), (224, 224), (64, 64), (20, 20), (130, 70), (96, 64)]
STEPS = (1, -2)
SEED = 11
BATCH = 3  # max_batch of most handles here: 4 frames at step 1 are two device batches (3 + 1 pairs)


def _frames(w, h, n=4):
    return SynthClip(w, h, SEED).frames(n)


def _stats_key(st):
    return (st.levels, [st.level_w[i] for i in range(st.levels)], [st.level_h[i] for i in range(st.levels)], st.batch)


def _flows(eng, w, h):
    """Everything the float entry point gives at w x h: per step the flows, the geometry dfx_get_stats reports and (TVL1)
    the iteration tables of the last batch and of the last pair."""
    out = {}
    for step in STEPS:
        fl = eng.calc_optflows(_frames(w, h), step)
        st = eng.stats()
        rec = {"flows": fl, "geom": _stats_key(st)}
        if eng.algorithm == "tvl1":
            rec["tables"] = eng.tvl1_batch_tables()
            rec["iters"] = st.iters_table()
        out[step] = rec
    return out


def _same(got, want, what):
    for step in STEPS:
        g, w = got[step], want[step]
        assert len(g["flows"]) == len(w["flows"]) > 0, what
        for i, (a, b) in enumerate(zip(g["flows"], w["flows"])):
            assert np.array_equal(a, b), (what, step, i, float(np.max(np.abs(a - b))))
        assert g["geom"] == w["geom"], (what, step)
        if "tables" in w:
            assert g["tables"] == w["tables"], (what, step)
            assert g["iters"] == w["iters"], (what, step)


_fresh_cache = {}


def _fresh(algo, w, h, **knobs):
    key = (algo, w, h, tuple(sorted(knobs.items())))
    if key not in _fresh_cache:
        with denseflow_amd.FlowEngine(w, h, algo, **knobs) as eng:
            _fresh_cache[key] = _flows(eng, w, h)
    return _fresh_cache[key]


@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_walk_matches_fresh_handles_and_allocates_once(algo):
    w0, h0 = WALK[0]
    with denseflow_amd.FlowEngine(w0, h0, algo, max_batch=BATCH) as eng:
        _same(_flows(eng, w0, h0), _fresh(algo, w0, h0, max_batch=BATCH), (algo, w0, h0))
        for w, h in WALK[1:]:
            eng.set_size(w, h)
            assert (eng.width, eng.height) == (w, h)
            _same(_flows(eng, w, h), _fresh(algo, w, h, max_batch=BATCH), (algo, w, h))
        # no hidden reallocation: every buffer has reached the largest stop's need, a second pass moves nothing
        held = eng.device_bytes()
        assert held > 0
        for w, h in WALK[1:]:
            eng.set_size(w, h)
            assert eng.device_bytes() == held, (algo, w, h)
            got = eng.calc_optflows(_frames(w, h), 1)
            assert eng.device_bytes() == held, (algo, w, h)
            assert all(np.array_equal(a, b) for a, b in zip(got, _fresh(algo, w, h, max_batch=BATCH)[1]["flows"]))


@pytest.mark.parametrize("impl", [0, 1])
def test_tvl1_impls_on_the_first_stops(impl):
    w0, h0 = WALK[0]
    with denseflow_amd.FlowEngine(w0, h0, "tvl1", max_batch=BATCH, impl=impl) as eng:
        for k, (w, h) in enumerate(WALK[:3]):
            if k:
                eng.set_size(w, h)
            _same(_flows(eng, w, h), _fresh("tvl1", w, h, max_batch=BATCH, impl=impl), (impl, w, h))


def test_tvl1_straggler_after_a_shrink():
    """A hard cut runs its levels to the iteration bound: the per-pair control state (Tvl1State, the done counter and the
    pinned done word) must start the FlowBuffer at the new size exactly as it does after create."""
    cut = ContentClip(65, 33, SEED, "cut").frames(2)
    easy = _frames(65, 33, 2)
    with denseflow_amd.FlowEngine(65, 33, "tvl1", max_batch=BATCH) as eng:
        eng.next_segments([2, 2])
        want = eng.calc_optflows(cut + easy, 1)
        want_tables = eng.tvl1_batch_tables()
    with denseflow_amd.FlowEngine(224, 224, "tvl1", max_batch=BATCH) as eng:
        eng.calc_optflows(_frames(224, 224), 1)
        eng.set_size(65, 33)
        eng.next_segments([2, 2])
        got = eng.calc_optflows(cut + easy, 1)
        assert eng.tvl1_batch_tables() == want_tables
    assert len(got) == len(want) == 2
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def _output_forms(eng, w, h):
    fr = _frames(w, h)
    u8 = eng.calc_optflows_u8(fr, 1, 20)
    png = eng.calc_optflows_png(fr, 1)
    png_s = eng.calc_optflows_png(fr, -2, submit=True)
    cap = int(eng._L.dfx_jpeg_capacity(eng._h))
    jpg = eng.calc_optflows_jpeg(fr, 1, 20)
    jpg80 = eng.calc_optflows_jpeg(fr, -2, 20, quality=80)
    enc = eng.encode_jpeg([fr[0], fr[1], fr[2]], 90)
    return {"u8": u8, "png": png, "png_submit": png_s, "cap": cap, "jpg": jpg, "jpg80": jpg80, "enc": enc}


def _same_forms(got, want, what):
    for k in ("u8", "png", "png_submit"):
        for a, b in zip(got[k][:2], want[k][:2]):
            assert len(a) == len(b) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b)), (what, k)
    for k in ("png", "png_submit"):
        assert np.array_equal(got[k][2], want[k][2]), (what, k, "bounds")
    assert got["cap"] == want["cap"], what
    for k in ("jpg", "jpg80"):
        assert got[k] == want[k] and len(got[k][0]) > 0, (what, k)  # lists of bytes: the files and with them their sizes
    assert got["enc"] == want["enc"] and len(got["enc"]) == 3, what


@pytest.mark.parametrize("algo", ["tvl1", "farn"])
def test_output_forms_after_resize(algo):
    want = {}
    for w, h in ((65, 33), (96, 64)):
        with denseflow_amd.FlowEngine(w, h, algo, max_batch=BATCH) as eng:
            want[(w, h)] = _output_forms(eng, w, h)
    with denseflow_amd.FlowEngine(96, 64, algo, max_batch=BATCH) as eng:
        _same_forms(_output_forms(eng, 96, 64), want[(96, 64)], (algo, "created"))
        eng.set_size(65, 33)
        _same_forms(_output_forms(eng, 65, 33), want[(65, 33)], (algo, "shrunk"))
        eng.set_size(96, 64)
        _same_forms(_output_forms(eng, 96, 64), want[(96, 64)], (algo, "back"))


@pytest.mark.parametrize("algo", ["tvl1", "brox"])
def test_submit_left_outstanding_is_complete_after_set_size(algo):
    want64 = _fresh(algo, 96, 64, max_batch=BATCH)[1]["flows"]
    want33 = _fresh(algo, 65, 33, max_batch=BATCH)[1]["flows"]
    with denseflow_amd.FlowEngine(96, 64, algo, max_batch=BATCH) as eng:
        t_f, flows = eng.submit_optflows(_frames(96, 64), 1)
        t_u, (ix, iy) = eng.submit_optflows(_frames(96, 64), 1, bound=20)
        eng.set_size(65, 33)  # nothing has been waited for: set_size does
        assert all(np.array_equal(a, b) for a, b in zip(flows, want64)) and len(flows) == len(want64)
        t2, flows33 = eng.submit_optflows(_frames(65, 33), 1)
        eng.wait(t_f)  # tickets from before the resize stay valid
        eng.wait(t_u)
        eng.wait(t2)
        assert all(np.array_equal(a, b) for a, b in zip(flows33, want33)) and len(flows33) == len(want33)
    with denseflow_amd.FlowEngine(96, 64, algo, max_batch=BATCH) as eng:
        rx, ry = eng.calc_optflows_u8(_frames(96, 64), 1, 20)
    assert all(np.array_equal(a, b) for a, b in zip(ix + iy, rx + ry))


def test_set_size_cancels_segments_and_source_format():
    with denseflow_amd.FlowEngine(96, 64, "farn", max_batch=BATCH) as eng:
        eng.set_source_format(48, 32, 1)
        eng._check(eng._L.dfx_next_segments(eng._h, (E.C.c_int * 2)(2, 2), 2))
        eng.set_size(65, 33)
        got = eng.calc_optflows(_frames(65, 33), 1)  # 65 x 33 gray frames, one clip of four: three pairs
    want = _fresh("farn", 65, 33, max_batch=BATCH)[1]["flows"]
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))


def _bgr(w, h, n=3):
    f = SynthClip(w, h, SEED).frames(n + 2)
    return [np.ascontiguousarray(np.stack([f[i], f[i + 1], f[i + 2]], -1)) for i in range(n)]


def test_frames_handle_follows_the_output_size():
    src = _bgr(96, 64)
    want = {}
    for w, h in ((48, 32), (33, 17)):
        with denseflow_amd.FlowEngine(w, h, "frames", max_batch=2) as eng:
            want[(w, h)] = (eng.extract_frames(src), eng.extract_frames(_bgr(w, h)), int(eng._L.dfx_jpeg_capacity_bgr(eng._h)))
    with denseflow_amd.FlowEngine(48, 32, "frames", max_batch=2) as eng:
        for w, h in ((48, 32), (33, 17), (48, 32)):
            eng.set_size(w, h)
            got = (eng.extract_frames(src), eng.extract_frames(_bgr(w, h)), int(eng._L.dfx_jpeg_capacity_bgr(eng._h)))
            assert got == want[(w, h)], (w, h)
            assert all(len(b) > 0 for b in got[0])
    with denseflow_amd.FlowEngine(96, 64, "tvl1", max_batch=BATCH) as eng:  # the colour stages of a flow handle
        eng.set_size(48, 32)
        assert eng.extract_frames(src) == want[(48, 32)][0]


def test_never_resized_handle_holds_the_same_memory():
    """Default batch (2048 pairs at these sizes): what dfx_create allocates at 96 x 64 is what a handle that went through
    20 x 20 and came back holds; nothing grew on the way and nothing was given up."""
    with denseflow_amd.FlowEngine(96, 64, "tvl1") as a, denseflow_amd.FlowEngine(96, 64, "tvl1") as b:
        created = a.device_bytes()
        assert created == b.device_bytes() > 0
        fa = a.calc_optflows(_frames(96, 64), 1)
        b.calc_optflows(_frames(96, 64), 1)
        b.set_size(20, 20)
        assert b.stats().batch == a.stats().batch == 2048
        small = b.calc_optflows(_frames(20, 20), 1)
        b.set_size(96, 64)
        fb = b.calc_optflows(_frames(96, 64), 1)
        assert a.device_bytes() == b.device_bytes() >= created
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    with denseflow_amd.FlowEngine(20, 20, "tvl1") as c:
        want = c.calc_optflows(_frames(20, 20), 1)
    assert all(np.array_equal(x, y) for x, y in zip(small, want)) and len(small) == 3


@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_failure_leaves_the_handle_intact(algo):
    want = _fresh(algo, 96, 64, max_batch=BATCH)[1]["flows"]
    with denseflow_amd.FlowEngine(96, 64, algo, max_batch=BATCH) as eng:
        held = eng.device_bytes()
        with pytest.raises(E.DfxError) as ei:
            eng.set_size(0, 5)
        assert ei.value.status == E.ERR_INVALID
        assert (eng.width, eng.height) == (96, 64)
        got = eng.calc_optflows(_frames(96, 64), 1)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == 3
        if algo == "tvl1":  # the 4 GiB pair-slot rule: refused while planning, before any allocation
            held = eng.device_bytes()
            with pytest.raises(E.DfxError) as ei:
                eng.set_size(8192, 8192)
            assert ei.value.status == E.ERR_INVALID
            assert eng.device_bytes() == held
            got = eng.calc_optflows(_frames(96, 64), 1)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == 3
            assert eng.stats().level_w[0] == 96 and eng.stats().level_h[0] == 64
