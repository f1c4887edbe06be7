"""The global-motion fit on the device (dfx_global_motion_device, denseflow_amd/csrc/global_motion_kernels.hip) against its
NumPy reference (tests/global_motion_ref.py): the twelve sums, valid, every inliers[k], status and rounds as integers, a and p
as bit patterns, the compensated flows as bit patterns, the moving masks byte for byte, the working words zero on return, and
every byte outside the windows of an output buffer still the fill.  Sizes are the smallest at which the kernels can go wrong:
the issue's four composed cases (97 x 61 and 130 x 97 are taller than one 32-row band and no multiple of it, 61 x 33 is one
row more than a band), 1100 x 70 for a fifth 256-column workgroup with a ragged right edge, 8192 x 8 for the largest terms
of the integer bound, one 1920 x 1080 pair of flows for a ticket that 272 workgroups take, and the layouts that select the
other access widths."""
import numpy as np
import pytest

from tests import global_motion_ref as R
from tests.devmem import DevBuf
from tests.test_global_motion_ref import CASES, FIRST, _case

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64


def _rec_dtype(dfx):
    from denseflow_amd import engine as E

    return E.GM_RESULT_DTYPE


class _Planes:
    """n x p planes of h rows of w elements in a device buffer with an explicit geometry (elements): lead, pitch, plane
    stride, item stride; GUARD elements in front and behind, every element outside the windows a fill."""

    def __init__(self, eng, n, p, h, w, dtype, fill, data=None, lead=0, pitch=None, plane=None, item=None):
        self.eng, self.n, self.p, self.h, self.w, self.dtype = eng, n, p, h, w, np.dtype(dtype)
        self.lead = lead
        self.pitch = w if pitch is None else pitch
        self.plane = h * self.pitch if plane is None else plane
        self.item = p * self.plane if item is None else item
        self.host = np.full(2 * GUARD + lead + n * self.item + 4, fill, self.dtype)
        self.outside = np.ones(self.host.shape, bool)
        for i in range(n):
            for k in range(p):
                win = self._win(self.host, i, k)
                if data is not None:
                    win[...] = data[i, k]
                self._win(self.outside, i, k)[...] = False
        self.fill = self.host.copy()
        self.dev = DevBuf(eng, init=self.host)

    def _win(self, buf, i, k):
        o = GUARD + self.lead + i * self.item + k * self.plane
        return buf[o:o + self.h * self.pitch].reshape(self.h, self.pitch)[:, :self.w]

    def ptr(self):
        return self.dev.ptr((GUARD + self.lead) * self.dtype.itemsize)

    def windows(self):
        buf = self.dev.get(self.dtype)
        wins = np.stack([np.stack([self._win(buf, i, k) for k in range(self.p)]) for i in range(self.n)])
        same = buf[self.outside].view(np.uint8) == self.fill[self.outside].view(np.uint8)
        return wins, bool(np.all(same))

    def untouched(self):
        return bool(np.array_equal(self.dev.get(self.dtype).view(np.uint8), self.fill.view(np.uint8)))

    def close(self):
        self.dev.close()


REC_FILL = 0xA5


class _Rig:
    """The device buffers of one batch of flows (n, 2, H, W) and optional masks (n, H, W) in one layout."""

    def __init__(self, dfx, eng, flows, masks=None, layout="dense", inplace=False):
        self.dfx, self.eng = dfx, eng
        self.flows, self.masks = flows, masks
        n, _, h, w = flows.shape
        self.n, self.h, self.w = n, h, w
        if layout == "dense":
            gf = gm = go = gv = {}
        elif layout == "scalar":  # a base one element in, a pitch of w + 4 (101 for 97): single elements everywhere
            gf = dict(lead=1, pitch=w + 4, plane=h * (w + 4) + 1, item=2 * (h * (w + 4) + 1) + 3)
            gm = gv = dict(lead=1, pitch=w + 2, item=h * (w + 2) + 1)
            go = dict(lead=3, pitch=w + 1, plane=h * (w + 1) + 2, item=2 * (h * (w + 1) + 2) + 1)
        else:  # "vector": every base and stride a multiple of 16 bytes, rows padded
            pw = (w + 3) // 4 * 4 + 4
            gf = go = dict(pitch=pw, plane=h * pw + 8, item=2 * (h * pw + 8) + 12)
            gm = gv = dict(pitch=pw, item=h * pw + 8)
        self.flow = _Planes(eng, n, 2, h, w, F32, np.nan, flows, **gf)
        self.mask = _Planes(eng, n, 1, h, w, np.uint8, 1, masks.reshape(n, 1, h, w), **gm) if masks is not None else None
        self.out = self.flow if inplace else _Planes(eng, n, 2, h, w, np.uint32, 0xA5A5A5A5, **go)
        self.moving = _Planes(eng, n, 1, h, w, np.uint8, 0xA5, **gv)
        self.rec_fill = np.full((n + 2) * _rec_dtype(dfx).itemsize, REC_FILL, np.uint8)
        self.rec = DevBuf(eng, init=self.rec_fill)
        self.bufs = [b for b in (self.flow, self.mask, self.out, self.moving) if b is not None]

    def call(self, model=1, rounds=5, thr=0.5, growth=2.0, want_out=True, want_moving=True, with_mask=True, **over):
        size = _rec_dtype(self.dfx).itemsize
        m = self.mask if with_mask else None
        kw = dict(d_flow_ptr=self.flow.ptr(), row_pitch_floats=self.flow.pitch, plane_stride_floats=self.flow.plane,
                  flow_stride_floats=self.flow.item, n=self.n, d_result_ptr=self.rec.ptr(size), model=model, rounds=rounds,
                  thr=thr, growth=growth, d_mask_ptr=m.ptr() if m else None, mask_pitch=m.pitch if m else 0,
                  mask_stride=m.item if m else 0, d_out_ptr=self.out.ptr() if want_out else None,
                  out_row_pitch_floats=self.out.pitch, out_plane_stride_floats=self.out.plane,
                  out_flow_stride_floats=self.out.item, d_moving_ptr=self.moving.ptr() if want_moving else None,
                  moving_pitch=self.moving.pitch, moving_stride=self.moving.item)
        kw.update(over)
        self.eng.global_motion_device(**kw)

    def records(self):
        """(the n records, whether the record in front of and the one behind them still hold the fill)."""
        dt = _rec_dtype(self.dfx)
        raw = self.rec.get(np.uint8)
        return raw[dt.itemsize:-dt.itemsize].view(dt), bool(np.all(raw[:dt.itemsize] == REC_FILL) and np.all(raw[-dt.itemsize:] == REC_FILL))

    def check(self, tag, model=1, rounds=5, thr=0.5, growth=2.0, want_out=True, want_moving=True, with_mask=True):
        self.call(model, rounds, thr, growth, want_out, want_moving, with_mask)
        refs = [R.global_motion(self.flows[i], self.masks[i] if self.masks is not None and with_mask else None, model, rounds,
                                thr, growth) for i in range(self.n)]
        rec, clean = self.records()
        assert clean, (tag, "a byte next to the records was written")
        for i, ref in enumerate(refs):
            t = (tag, i)
            assert np.array_equal(rec["sums"][i], ref["sums"]), (t, rec["sums"][i], ref["sums"])
            assert rec["valid"][i] == ref["valid"], (t, rec["valid"][i], ref["valid"])
            assert np.array_equal(rec["inliers"][i], ref["inliers"]), (t, rec["inliers"][i], ref["inliers"])
            assert rec["status"][i] == ref["status"] and rec["rounds"][i] == rounds, (t, rec["status"][i], ref["status"])
            assert np.array_equal(rec["a"][i].view(np.uint64), ref["a"].view(np.uint64)), (t, rec["a"][i], ref["a"])
            assert np.array_equal(rec["p"][i].view(np.uint32), ref["p"].view(np.uint32)), (t, rec["p"][i], ref["p"])
            assert np.all(rec["work"][i] == 0), (t, "the working words are not zero on return")
        if want_out:
            got, clean = self.out.windows()
            want = np.stack([r["out"] for r in refs]).view(np.uint32)
            bad = got.view(np.uint32) != want
            assert not bad.any(), (tag, int(bad.sum()), got.view(np.uint32)[bad][:4], want[bad][:4])
            assert clean, (tag, "an element outside the windows of out was written")
        elif self.out is not self.flow:
            assert self.out.untouched(), (tag, "out was written without being asked for")
        if want_moving:
            got, clean = self.moving.windows()
            assert np.array_equal(got[:, 0], np.stack([r["moving"] for r in refs])), tag
            assert clean, (tag, "a byte outside the windows of moving was written")
        else:
            assert self.moving.untouched(), (tag, "moving was written without being asked for")
        if self.out is not self.flow or not want_out:
            assert self.flow.untouched(), (tag, "the flows were written")
        if self.mask is not None:
            assert self.mask.untouched(), (tag, "the masks were written")
        return refs

    def reset(self):
        e = self.eng
        for b in (self.out, self.moving):
            e._check(e._L.dfx_memcpy_h2d(e._h, b.dev.ptr(), b.fill.ctypes.data, b.fill.nbytes))
        e._check(e._L.dfx_memcpy_h2d(e._h, self.rec.ptr(), self.rec_fill.ctypes.data, self.rec_fill.nbytes))

    def close(self):
        for b in self.bufs:
            b.close()
        self.rec.close()


def _flows(key):
    return np.array(_case(key)[0])[None]


@pytest.mark.parametrize("model", [R.TRANSLATION, R.AFFINE])
@pytest.mark.parametrize("key", list(CASES))
def test_the_composed_cases_in_both_models(dfx, key, model):
    w, h = key[:2]
    with dfx.FlowEngine(w, h, "farn") as eng:
        rig = _Rig(dfx, eng, _flows(key))
        try:
            refs = rig.check((key, model), model=model)
        finally:
            rig.close()
    counts = CASES[key][0]
    if model == R.AFFINE and counts is not None:  # the reference test's table, now from the device's twin
        assert [int(c) for c in refs[0]["inliers"][:5]] == counts


def _three():
    """Three different 97 x 61 flows and masks: the two composed cases and the first with special values planted."""
    a, b = np.array(_case(FIRST)[0]), np.array(_case((97, 61, 9, 6, 0.45, 0.05))[0])
    c = a[:, ::-1, ::-1].copy()
    c[0, 3, 5], c[1, 7, 9], c[0, 11, 2], c[1, 60, 96], c[0, 0, 0] = np.nan, np.inf, 5000.0, -np.inf, -4096.0
    flows = np.stack([a, b, c])
    masks = (np.random.default_rng(7).random((3, 61, 97)) < 0.2).astype(np.uint8)
    masks[1] = (~_case((97, 61, 9, 6, 0.45, 0.05))[1]).astype(np.uint8)
    return flows, masks


@pytest.mark.parametrize("layout", ["dense", "scalar", "vector"])
def test_three_flows_in_one_call_in_every_layout(dfx, layout):
    """Per-flow indexing and tickets; with "scalar", 97 wide with row_pitch_floats = 101 and a base one float in."""
    flows, masks = _three()
    with dfx.FlowEngine(97, 61, "tvl1") as eng:
        rig = _Rig(dfx, eng, flows, masks, layout)
        try:
            if layout == "scalar":
                assert rig.flow.pitch == 101 and rig.flow.lead == 1 and rig.flow.ptr() % 16 == 4
            refs = rig.check((layout, "masks"))
            ok = R.ok_of(flows[2])  # the five planted values fail the test on their own
            assert ok.sum() == 97 * 61 - 5 and refs[2]["valid"] == (ok & (masks[2] == 0)).sum()
            assert np.isnan(refs[2]["out"]).sum() == 1
            rig.reset()
            rig.check((layout, "no masks", "translation"), model=R.TRANSLATION, rounds=3, thr=1.0, growth=1.5, with_mask=False)
        finally:
            rig.close()


def test_special_values_are_excluded_and_nan_propagates(dfx):
    flows, _ = _three()
    plain = np.array(_case(FIRST)[0])[:, ::-1, ::-1].copy()
    with dfx.FlowEngine(97, 61, "brox") as eng:
        rig = _Rig(dfx, eng, np.stack([plain, flows[2]]))
        try:
            refs = rig.check("specials")
            got = rig.out.windows()[0].view(F32)
        finally:
            rig.close()
    assert refs[0]["valid"] == 97 * 61 and refs[1]["valid"] == 97 * 61 - 5
    assert np.isnan(got[1, 0, 3, 5]) and got[1, 1, 7, 9] == np.inf and got[1, 1, 60, 96] == -np.inf
    for y, x in ((3, 5), (7, 9), (11, 2), (60, 96), (0, 0)):
        assert refs[1]["moving"][y, x] == 1


def test_a_second_call_into_the_same_records(dfx):
    """The library zeroes the records: a call on top of another call's results, and on top of garbage, gives the same."""
    flows, masks = _three()
    with dfx.FlowEngine(97, 61, "farn") as eng:
        rig = _Rig(dfx, eng, flows, masks, "vector")
        try:
            rig.check("first")
            first = rig.records()[0].copy()
            rig.check("second, other settings", model=R.TRANSLATION, rounds=8, thr=0.25, growth=1.25)
            rig.check("third")
            assert np.array_equal(rig.records()[0].view(np.uint8), first.view(np.uint8))
        finally:
            rig.close()


def test_in_place_and_every_combination_of_outputs(dfx):
    flows, masks = _three()
    with dfx.FlowEngine(97, 61, "farn") as eng:
        for layout in ("dense", "scalar"):
            rig = _Rig(dfx, eng, flows, masks, layout)
            try:
                for want_out, want_moving in ((True, False), (False, True), (False, False), (True, True)):
                    rig.reset()
                    rig.check((layout, want_out, want_moving), want_out=want_out, want_moving=want_moving)
            finally:
                rig.close()
            rig = _Rig(dfx, eng, flows, masks, layout, inplace=True)
            try:
                refs = [R.global_motion(flows[i], masks[i]) for i in range(3)]
                rig.call()
                got, clean = rig.flow.windows()
                assert clean, "in place: an element outside the windows was written"
                assert np.array_equal(got.view(np.uint32), np.stack([r["out"] for r in refs]).view(np.uint32))
                assert np.array_equal(rig.moving.windows()[0][:, 0], np.stack([r["moving"] for r in refs]))
                rec = rig.records()[0]
                assert np.array_equal(rec["a"].view(np.uint64), np.stack([r["a"] for r in refs]).view(np.uint64))
            finally:
                rig.close()


def test_the_degenerate_rounds_keep_the_first_model(dfx):
    with dfx.FlowEngine(97, 61, "farn") as eng:
        rig = _Rig(dfx, eng, _flows(FIRST))
        try:
            refs = rig.check("rounds 3", rounds=3)
            rec = rig.records()[0].copy()
            rig.reset()
            rig.check("rounds 1", rounds=1)
            one = rig.records()[0]
        finally:
            rig.close()
    assert refs[0]["status"] == 6 and rec["status"][0] == 6 and list(rec["inliers"][0][:3]) == [5917, 0, 0]
    assert np.array_equal(rec["a"].view(np.uint64), one["a"].view(np.uint64)) and np.all(rec["sums"] == 0)


def test_wider_than_a_workgroup_and_a_ragged_last_band(dfx):
    """1100 x 70: five workgroup columns, the last with 76 columns, and three bands, the last with 6 rows."""
    w, h = 1100, 70
    rng = np.random.default_rng(1100)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u = 1.75 + 0.002 * x - 0.011 * y + rng.normal(0, 0.1, (h, w))
    v = -0.5 + 0.004 * x + 0.003 * y + rng.normal(0, 0.1, (h, w))
    u[20:50, 700:1000], v[20:50, 700:1000] = -6.0, 3.0
    flows = np.stack([u, v]).astype(F32)[None]
    mask = (rng.random((1, h, w)) < 0.1).astype(np.uint8)
    with dfx.FlowEngine(w, h, "farn") as eng:
        for layout in ("dense", "scalar"):
            rig = _Rig(dfx, eng, flows, mask, layout)
            try:
                refs = rig.check(("1100x70", layout))
            finally:
                rig.close()
    a = refs[0]["a"]
    assert abs(a[0] - 1.75) < 0.01 and abs(a[1] - 0.002) < 1e-4 and abs(a[5] - 0.003) < 1e-4, a


def test_a_1080p_flows_272_workgroups_take_one_ticket(dfx):
    """1920 x 1080, two flows: 272 workgroups per flow, spread over every XCD, add to one record and take one ticket — the
    size the measurements are made at, and the most workgroups per flow of any case here."""
    w, h = 1920, 1080
    rng = np.random.default_rng(1080)
    x, y = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    flows = np.stack([np.stack([1.5 + 0.001 * x - 0.002 * y, -0.75 + 0.002 * x + 0.001 * y]),
                      np.stack([-3 + 0.0005 * y, 2 - 0.0007 * x])]).astype(F32)
    flows += rng.normal(0, 0.2, flows.shape).astype(F32)
    flows[:, :, 300:700, 500:1200] += F32(5.0)
    with dfx.FlowEngine(w, h, "farn") as eng:
        rig = _Rig(dfx, eng, flows)
        try:
            refs = rig.check("1080p", rounds=3)
        finally:
            rig.close()
    for r in refs:
        assert r["status"] == 0 and r["inliers"][0] == w * h and 0.7 * w * h < r["inliers"][2] < 0.8 * w * h, r["inliers"]


def test_the_largest_terms_of_the_integer_bound(dfx):
    """8192 x 8 with u = +-4095.99 in the corners (|xc| = 8191, |q| = 2^20 - 3) over a large smooth flow."""
    w, h = 8192, 8
    x = np.arange(w, dtype=np.float64)[None, :] - (w - 1) / 2
    y = np.arange(h, dtype=np.float64)[:, None] - (h - 1) / 2
    u, v = (0.9 * x + 3.0 * y).astype(F32), (-0.7 * x + 11.0 * y).astype(F32)
    big = F32(4095.99)
    u[0, 0], u[0, -1], u[-1, 0], u[-1, -1] = big, -big, -big, big
    v[0, 0], v[0, -1], v[-1, 0], v[-1, -1] = -big, big, big, -big
    flows = np.stack([u, v])[None]
    assert np.abs(flows).max() < 4096 and int(np.rint(big * F32(256.0))) == 2 ** 20 - 3
    with dfx.FlowEngine(w, h, "farn") as eng:
        rig = _Rig(dfx, eng, flows)
        try:
            refs = rig.check("8192x8 plain", rounds=1)
            rig.reset()
            rig.check("8192x8 robust", rounds=4, thr=2.0, growth=4.0)
        finally:
            rig.close()
    s = refs[0]["sums"]
    assert s[0] == w * h and s[1] == 0 and s[2] == 0 and s[3] > 2 ** 40 and abs(int(s[7])) > 2 ** 45, s


def test_numpy_wrapper(dfx):
    flows, masks = _three()
    refs = [R.global_motion(flows[i], masks[i], R.AFFINE, 4, 0.75, 1.5) for i in range(3)]
    with dfx.FlowEngine(97, 61, "tvl1") as eng:
        before = eng.device_bytes()
        params, comp, moving, info = eng.global_motion(flows, mask=masks, model="affine", rounds=4, thr=0.75, growth=1.5)
        assert eng.device_bytes() == before
        assert eng.stats().pairs == 0
        empty = eng.global_motion(np.zeros((0, 2, 61, 97), F32))
    assert params.dtype == np.float64 and params.shape == (3, 6)
    assert np.array_equal(params.view(np.uint64), np.stack([r["a"] for r in refs]).view(np.uint64))
    assert np.array_equal(comp.view(np.uint32), np.stack([r["out"] for r in refs]).view(np.uint32))
    assert np.array_equal(moving, np.stack([r["moving"] for r in refs]))
    assert np.array_equal(info["inliers"], np.stack([r["inliers"] for r in refs]))
    assert np.array_equal(info["valid"], np.array([r["valid"] for r in refs], np.uint64))
    assert np.array_equal(info["status"], np.array([r["status"] for r in refs], np.uint32)) and np.all(info["rounds"] == 4)
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 2, 61, 97) and empty[2].shape == (0, 61, 97)


def test_torch_wrapper_on_a_non_contiguous_slice(dfx):
    import torch

    flows, masks = _three()
    refs = [R.global_motion(flows[i], masks[i]) for i in range(3)]
    want_out = np.stack([r["out"] for r in refs]).view(np.uint32)
    dev = torch.device("cuda", 0)
    big = torch.full((3, 2, 61 + 2, 97 + 7), float("nan"), device=dev)
    big[:, :, 1:62, 3:100] = torch.from_numpy(flows).to(dev)
    view = big[:, :, 1:62, 3:100]
    big_mask = torch.ones((3, 61 + 1, 97 + 3), dtype=torch.uint8, device=dev)
    big_mask[:, :61, 2:99] = torch.from_numpy(masks).to(dev)
    with dfx.FlowEngine(97, 61, "farn") as eng:
        params, comp, moving, info = eng.global_motion_tensor(view, mask=big_mask[:, :61, 2:99])
        assert comp.is_contiguous() and comp.shape == (3, 2, 61, 97) and moving.dtype == torch.uint8
        assert np.array_equal(comp.cpu().numpy().view(np.uint32), want_out)
        assert np.array_equal(moving.cpu().numpy(), np.stack([r["moving"] for r in refs]))
        assert params.dtype == torch.float64
        assert np.array_equal(params.cpu().numpy().view(np.uint64), np.stack([r["a"] for r in refs]).view(np.uint64))
        assert np.array_equal(info["inliers"].numpy().astype(np.uint64), np.stack([r["inliers"] for r in refs]))
        assert np.array_equal(info["status"].numpy(), np.array([r["status"] for r in refs]))
        # in place, into the slice itself: nothing outside it changes
        _, same, none, _ = eng.global_motion_tensor(view, mask=big_mask[:, :61, 2:99], out=view, want_moving=False)
        assert same.data_ptr() == view.data_ptr() and none is None
        assert np.array_equal(view.contiguous().cpu().numpy().view(np.uint32), want_out)
        frame = torch.ones_like(big, dtype=torch.bool)
        frame[:, :, 1:62, 3:100] = False
        assert bool(torch.isnan(big[frame]).all()), "written outside the slice"


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    flows, masks = _three()
    w, h = 97, 61
    nan, inf = float("nan"), float("inf")
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        rig = _Rig(dfx, eng, flows, masks)
        try:
            refused = [dict(d_flow_ptr=None), dict(d_result_ptr=None), dict(d_result_ptr=rig.rec.ptr(4)), dict(n=-1),
                       dict(model=-1), dict(model=2), dict(rounds=0), dict(rounds=9), dict(rounds=-3),
                       dict(thr=0.0), dict(thr=-1.0), dict(thr=nan), dict(thr=inf),
                       dict(growth=0.99), dict(growth=nan), dict(growth=inf), dict(growth=-2.0),
                       dict(row_pitch_floats=w - 1), dict(plane_stride_floats=w * h - 1), dict(flow_stride_floats=2 * w * h - 1),
                       dict(mask_pitch=w - 1), dict(mask_stride=w * h - 1),
                       dict(out_row_pitch_floats=w - 1), dict(out_plane_stride_floats=w * h - 1),
                       dict(out_flow_stride_floats=2 * w * h - 1), dict(moving_pitch=w - 1), dict(moving_stride=w * h - 1)]
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    rig.call(**kw)
                assert e.value.status == 1, kw
            with pytest.raises(dfx.DfxError) as e:  # a NULL descriptor
                eng._check(eng._L.dfx_global_motion_device(eng._h, None))
            assert e.value.status == 1
            assert rig.out.untouched() and rig.moving.untouched(), "a refused call wrote"
            assert np.all(rig.rec.get(np.uint8) == REC_FILL), "a refused call wrote"
            rig.call(n=0)  # DFX_OK, launches nothing
            eng.global_motion_device(None, 0, 0, 0, 0, None, model=9, rounds=0, thr=nan, growth=nan)  # n = 0: nothing else is looked at
            assert rig.out.untouched() and rig.moving.untouched() and np.all(rig.rec.get(np.uint8) == REC_FILL), "n = 0 wrote"
            # the strides of absent buffers are not looked at
            rig.call(want_out=False, want_moving=False, with_mask=False, out_row_pitch_floats=0, moving_pitch=0)
            rig.reset()
            rig.check("after the refusals")
        finally:
            rig.close()
    with dfx.FlowEngine(w, h, "frames") as eng:
        rig = _Rig(dfx, eng, flows, masks)
        try:
            with pytest.raises(dfx.DfxError) as e:
                rig.call()
            assert e.value.status == 4
            assert rig.out.untouched() and rig.moving.untouched() and np.all(rig.rec.get(np.uint8) == REC_FILL)
        finally:
            rig.close()
