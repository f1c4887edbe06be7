"""Caller-supplied initial flows for -a=tvl1 on the device (dfx_calc_batch_init*, FlowEngine(..., init=)): the seed chain
kernel, the seeded coarsest level in every kernel form, and every entry point, against tests/initial_flow_ref.py.  The
device arithmetic is the reference's operation for operation, so every comparison is np.array_equal of the flows AND
equality of the executed inner-iteration table and the number of convergence sums evaluated.

Inputs: frames 0, 6, 12, 18 of a SynthClip (three pairs of about 10 px of motion), max_batch = 2 (a full batch and a ragged
one), seeds zeros / true flow / half the true flow.  Shapes as in tests/test_tvl1_gamma_gpu.py: 97x61 (a second tile of 33
columns), 130x97 (a third tile of two columns), 65x17 (one level), 65x33 (two levels).  Before an engine is touched every
case asserts on reference output that the seeded flows of pairs 1 and 2 differ from the unseeded ones by more than
1e-3 px.  No case feeds non-finite or out-of-domain seeds to the device."""
import numpy as np
import pytest

from tests import initial_flow_ref as IR

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
DISCRIMINATION = 1e-3  # px
SIZES = {(97, 61): 9, (130, 97): 5, (65, 17): 4, (65, 33): 4}  # (w, h) -> SynthClip seed
SET_F = dict(scale_step=0.6, nscales=6)
_ENGINE_NAME = dict(scale_step="tvl1_scale_step", nscales="tvl1_nscales", gamma="tvl1_gamma")

_inputs, _refs = {}, {}


def _in(w, h):
    if (w, h) not in _inputs:
        _inputs[(w, h)] = IR.seeded_inputs(w, h, SIZES[(w, h)])
    return _inputs[(w, h)]


def _engine_kw(ref_kw):
    return {_ENGINE_NAME[k]: v for k, v in ref_kw.items()}


def _ref(oracle, w, h, seeded=True, **ref_kw):
    """(flow, table, checks) of the three pairs, computed once per case and never changed."""
    key = (w, h, seeded, tuple(sorted(ref_kw.items())))
    if key not in _refs:
        frames, seeds = _in(w, h)
        out = []
        for i in range(3):
            r = IR.tvl1_init_calc(oracle, frames[i], frames[i + 1], seeds[i] if seeded else None, **ref_kw)
            r[0].setflags(write=False)
            out.append(r)
        _refs[key] = out
    return _refs[key]


def _discriminates(oracle, w, h, **ref_kw):
    ref, base = _ref(oracle, w, h, True, **ref_kw), _ref(oracle, w, h, False, **ref_kw)
    diffs = [float(np.max(np.abs(a[0] - b[0]))) for a, b in zip(ref, base)]
    print(f"tvl1 {w}x{h} {ref_kw}: seeded against unseeded reference, max-abs per pair {diffs}; inner iterations seeded "
          f"{[sum(map(sum, r[1])) for r in ref]} unseeded {[sum(map(sum, r[1])) for r in base]}")
    assert all(np.isfinite(r[0]).all() for r in ref)
    assert np.array_equal(ref[0][0], base[0][0])  # pair 0: the zero seed
    assert min(diffs[1:]) > DISCRIMINATION, (w, h, diffs)


def _table(st, warps=5):
    return [r[:warps] for r in st.iters_table()]


def _same(got, ref, what):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g, r[0]), f"{what}: pair {i} differs, max-abs {np.max(np.abs(g - r[0]))}"


def _check(dfx, oracle, w, h, form_kw, **ref_kw):
    _discriminates(oracle, w, h, **ref_kw)
    ref = _ref(oracle, w, h, True, **ref_kw)
    frames, seeds = _in(w, h)
    with dfx.FlowEngine(w, h, "tvl1", max_batch=2, **_engine_kw(ref_kw), **form_kw) as eng:
        first = eng.calc(frames[1], frames[2], init=seeds[1])  # the handle's first call is a seeded one
        st = eng.stats()
        assert np.array_equal(first, ref[1][0]), f"calc(init=): max-abs {np.max(np.abs(first - ref[1][0]))}"
        assert _table(st) == ref[1][1] and st.tvl1_checks == ref[1][2]
        flows = eng.calc_optflows(frames, 1, init=seeds)  # 3 pairs: a batch of two and a ragged one
        st = eng.stats()
    _same(flows, ref, f"tvl1 {w}x{h} {form_kw} {ref_kw}")
    assert _table(st) == ref[2][1], "inner-iteration counts differ from the reference (last pair)"
    assert st.tvl1_checks == ref[2][2]


def _forms():
    from denseflow_amd import engine as E

    return {"tuned": dict(), "impl1": dict(impl=1), "impl2": dict(impl=2), "no_head": dict(variant=E.VAR_TVL1_NO_HEAD),
            "warp_gather": dict(variant=E.VAR_TVL1_WARP_GATHER),
            "nbr_lds": dict(variant=E.VAR_TVL1_HEAD_NBR_LDS | E.VAR_TVL1_STEP_NBR_LDS)}


@pytest.mark.parametrize("form", ["tuned", "impl1"])
@pytest.mark.parametrize("w,h", list(SIZES))
def test_seeded_flows_match_the_reference(dfx, oracle, w, h, form):
    _check(dfx, oracle, w, h, _forms()[form])


@pytest.mark.parametrize("form", ["impl2", "no_head", "warp_gather", "nbr_lds"])
@pytest.mark.parametrize("w,h", [(97, 61), (130, 97)])
def test_every_kernel_form(dfx, oracle, w, h, form):
    _check(dfx, oracle, w, h, _forms()[form])


@pytest.mark.parametrize("form", ["tuned", "impl1"])
@pytest.mark.parametrize("w,h", [(97, 61), (130, 97)])
def test_one_level_starts_far_beyond_the_warp_tiles_halo(dfx, oracle, w, h, form):
    """nscales = 1: level 0 starts with displacements up to 9 px, so the head kernel's `far` gather does most pixels."""
    _, seeds = _in(w, h)
    assert float(np.max(np.abs(seeds[1]))) > 6.0
    _check(dfx, oracle, w, h, _forms()[form], nscales=1)


def test_non_default_pyramid(dfx, oracle):
    _check(dfx, oracle, 130, 97, dict(), **SET_F)


@pytest.mark.parametrize("form", ["tuned", "impl1"])
def test_seed_on_a_gamma_handle(dfx, oracle, form):
    _check(dfx, oracle, 97, 61, _forms()[form], gamma=0.4)


def test_every_entry_point(dfx, oracle):
    import torch

    w, h = 130, 97
    _discriminates(oracle, w, h)
    ref = _ref(oracle, w, h)
    frames, seeds = _in(w, h)
    want = np.stack([r[0] for r in ref])
    with dfx.FlowEngine(w, h, "tvl1", max_batch=2) as eng:
        # the device form with the seed buffer identical to the output buffer
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        buf = torch.from_numpy(np.stack(seeds)).cuda()
        torch.cuda.synchronize()
        eng.calc_optflows_device(d_frames.data_ptr(), w, w * h, 4, 1, buf.data_ptr(), w * h * 2, init=buf.data_ptr())
        assert np.array_equal(buf.cpu().numpy(), want), "device form, in place"
        st = eng.stats()
        assert _table(st) == ref[2][1] and st.tvl1_checks == ref[2][2]
        # the host form with padded seed rows: init_pitch = W * 8 + 64
        padded = [np.full((h, 2 * w + 16), np.float32(-777.25)) for _ in seeds]
        views = [p[:, :2 * w].reshape(h, w, 2) for p in padded]
        for v, s in zip(views, seeds):
            v[...] = s
        assert views[0].strides[0] == w * 8 + 64
        _same(eng.calc_optflows(frames, 1, init=views), ref, "host form, padded seed rows")
        # flow_tensor, raw and bounded (the seed is raw pixels either way), out-of-place and in place
        planes = torch.from_numpy(np.stack(seeds).transpose(0, 3, 1, 2).copy()).cuda()
        raw = eng.flow_tensor(d_frames, 1, init=planes)
        assert np.array_equal(raw.cpu().numpy(), want.transpose(0, 3, 1, 2)), "flow_tensor raw"
        bounded = eng.flow_tensor(d_frames, 1, bound=20, init=planes)
        assert np.array_equal(bounded.cpu().numpy(),
                              np.clip(want.transpose(0, 3, 1, 2), np.float32(-20), np.float32(20)) / np.float32(20))
        inplace = planes.clone()
        eng.flow_tensor(d_frames, 1, out=inplace, init=inplace)
        assert np.array_equal(inplace.cpu().numpy(), want.transpose(0, 3, 1, 2)), "flow_tensor in place"
        # two clips in one call: [f0, f1] and [f1, f2, f3] -> pairs (0, 1), (1, 2), (2, 3), seeds in clip order
        eng.next_segments([2, 3])
        seg = eng.calc_optflows([frames[0], frames[1], frames[1], frames[2], frames[3]], 1, init=seeds)
        _same(seg, ref, "next_segments([2, 3])")
        # after set_size: another size and back
        w2, h2 = 65, 33
        frames2, seeds2 = _in(w2, h2)
        eng.set_size(w2, h2)
        _same(eng.calc_optflows(frames2, 1, init=seeds2), _ref(oracle, w2, h2), "after set_size(65, 33)")
        eng.set_size(w, h)
        _same(eng.calc_optflows(frames, 1, init=seeds), ref, "after set_size back")


def test_no_state_leaks_between_seeded_and_unseeded_calls(dfx, oracle):
    w, h = 97, 61
    _discriminates(oracle, w, h)
    ref, base = _ref(oracle, w, h, True), _ref(oracle, w, h, False)
    frames, seeds = _in(w, h)
    for form_kw in (dict(), dict(impl=1)):
        with dfx.FlowEngine(w, h, "tvl1", max_batch=2, **form_kw) as eng:
            _same(eng.calc_optflows(frames, 1, init=seeds), ref, "seeded")
            _same(eng.calc_optflows(frames, 1), base, "unseeded after seeded")
            st = eng.stats()
            assert _table(st) == base[2][1] and st.tvl1_checks == base[2][2]
            _same(eng.calc_optflows(frames, 1, init=seeds), ref, "seeded after unseeded")


def test_refusals_leave_the_handle_usable_and_unseeded_handles_hold_no_seed_staging(dfx, oracle):
    import ctypes as C

    w, h = 97, 61
    ref, base = _ref(oracle, w, h, True), _ref(oracle, w, h, False)
    frames, seeds = _in(w, h)
    with dfx.FlowEngine(w, h, "brox") as eng:
        with pytest.raises(dfx.DfxError) as e:
            eng.calc(frames[0], frames[1], init=seeds[1])
        assert e.value.status == UNSUPPORTED
        assert np.isfinite(eng.calc(frames[0], frames[1])).all()
    L = dfx.load_library()
    with dfx.FlowEngine(w, h, "frames") as eng:  # a DFX_ALGO_FRAMES handle computes no flow
        with pytest.raises(dfx.DfxError) as e:
            eng.calc_optflows(frames, 1, init=seeds)
        assert e.value.status == UNSUPPORTED
        assert L.dfx_calc_batch_init_device(eng._h, None, w, w * h, 4, 1, None, w * h * 2, None, w * h * 2) == UNSUPPORTED
        assert L.dfx_calc_batch_planar_init_device(eng._h, None, w, w * h, 4, 1, 0.0, None, None, w, w * h, 2 * w * h) == UNSUPPORTED
    with dfx.FlowEngine(w, h, "tvl1", max_batch=2) as fresh, dfx.FlowEngine(w, h, "tvl1", max_batch=2) as eng:
        _same(eng.calc_optflows(frames, 1), base, "unseeded")
        fresh.calc_optflows(frames, 1)
        assert eng.device_bytes() == fresh.device_bytes()
        fp = (C.c_void_p * 4)(*[f.ctypes.data for f in frames])
        out = [np.empty((h, w, 2), np.float32) for _ in range(3)]
        op = (C.c_void_p * 3)(*[o.ctypes.data for o in out])
        ip = (C.c_void_p * 3)(*[s.ctypes.data for s in seeds])
        assert L.dfx_calc_batch_init(eng._h, fp, w, 4, 1, None, w * 8, op, w * 8) == INVALID  # NULL seed
        assert L.dfx_calc_batch_init(eng._h, fp, w, 4, 1, ip, w * 8 - 4, op, w * 8) == INVALID  # short pitch
        assert L.dfx_calc_batch_init_device(eng._h, None, w, w * h, 4, 1, None, w * h * 2, None, w * h * 2) == INVALID
        # the device forms, with real device buffers: a short seed stride, and the planar form's own refusals
        import torch

        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        d_seed = torch.from_numpy(np.stack(seeds)).cuda()
        d_out = torch.full((3, h, w, 2), -777.25, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        fr, sd, ot, n2 = d_frames.data_ptr(), d_seed.data_ptr(), d_out.data_ptr(), w * h * 2
        assert L.dfx_calc_batch_init_device(eng._h, fr, w, w * h, 4, 1, sd, n2 - 1, ot, n2) == INVALID  # init_stride_floats
        assert L.dfx_calc_batch_init_device(eng._h, fr, w, w * h, 4, 1, sd, n2, ot, n2 - 1) == INVALID  # as the unseeded twin
        planar = L.dfx_calc_batch_planar_init_device
        assert planar(eng._h, fr, w, w * h, 4, 1, 0.0, None, ot, w, w * h, n2) == INVALID  # NULL seed
        assert planar(eng._h, fr, w, w * h, 4, 1, -1.0, sd, ot, w, w * h, n2) == INVALID  # norm_bound
        assert planar(eng._h, fr, w, w * h, 4, 1, 0.0, sd, ot, w - 1, w * h, n2) == INVALID  # row pitch below W
        assert planar(eng._h, fr, w, w * h, 4, 1, 0.0, sd, ot, w, w * h - 1, n2) == INVALID  # planes overlap
        assert planar(eng._h, fr, w, w * h, 4, 1, 0.0, sd, ot, w, w * h, n2 - 1) == INVALID  # flows overlap
        assert planar(eng._h, fr, w - 1, w * h, 4, 1, 0.0, sd, ot, w, w * h, n2) == INVALID  # frame pitch
        torch.cuda.synchronize()
        assert bool((d_out == -777.25).all()), "a refused call wrote to the output"
        assert eng.device_bytes() == fresh.device_bytes(), "a refused seeded call allocated seed staging"
        _same(eng.calc_optflows(frames, 1), base, "unseeded after the refusals")
        assert eng.device_bytes() == fresh.device_bytes()
        _same(eng.calc_optflows(frames, 1, init=seeds), ref, "seeded after the refusals")
        # the host form's staging pair: max_batch dense seeds per set, allocated by the first seeded call
        assert eng.device_bytes() - fresh.device_bytes() == 2 * 2 * w * h * 8
