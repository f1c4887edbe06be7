"""RGB order and channels-first sources (dfx_set_source_format_ex, dfx_prepare_frames_layout*, order= / layout= of
set_source_format, prepare_frames and flow_tensor): the gray frame — and with it every flow — is what the BGR interleaved
path gives for the same picture rearranged on the host, byte for byte.  Geometries: a general resize, the exact 2x
decimation and the copy branch of the preparation kernel."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

W, H = 67, 35
GEOMS = [(80, 44), (134, 70), (67, 35)]  # source sizes: general resize, exact 2x, copy
N_FRAMES, MAX_BATCH = 8, 3
ORDERS, LAYOUTS = ["bgr", "rgb"], ["hwc", "chw"]
SENT = 0xA7

_bgr_cache = {}


def _bgr(ws, hs):
    """The colour frames of tests/test_planar_gpu.py::test_flow_tensor_bgr_source_segments_and_set_size, BGR interleaved."""
    if (ws, hs) not in _bgr_cache:
        rng = np.random.default_rng(11)
        gray = SynthClip(ws, hs, 9).frames(N_FRAMES)
        fr = [np.stack([g, np.roll(g, 1, 1), 255 - g], -1) + rng.integers(0, 2, (hs, ws, 3), dtype=np.uint8) for g in gray]
        for f in fr:
            f.setflags(write=False)
        _bgr_cache[(ws, hs)] = fr
    return _bgr_cache[(ws, hs)]


def _arranged(bgr, order, layout):
    """The same picture in the given channel order and layout."""
    f = bgr[..., ::-1] if order == "rgb" else bgr
    return np.ascontiguousarray(f.transpose(2, 0, 1) if layout == "chw" else f)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("ws,hs", GEOMS)
def test_prepare_frames_is_the_oracle_on_the_bgr_picture(dfx, oracle, ws, hs, order, layout):
    import torch

    bgr = _bgr(ws, hs)[:3]
    want = [oracle.prepare_frame(np.ascontiguousarray(f), W, H) for f in bgr]
    src = [_arranged(f, order, layout) for f in bgr]
    n = len(src)
    with dfx.FlowEngine(W, H, "tvl1", max_batch=MAX_BATCH) as eng:
        host = eng.prepare_frames(src, order=order, layout=layout)
        for g, r in zip(host, want):
            assert np.array_equal(g, r)
        # the device form, rows (and, channels-first, planes) padded, frames padded: only the gray windows are written
        if layout == "chw":
            pitch, plane_stride = ws + 5, (ws + 5) * hs + 13
            frame_stride = 3 * plane_stride + 7
            buf = np.full(n * frame_stride, 0x33, np.uint8)
            for i, f in enumerate(src):
                for c in range(3):
                    o = i * frame_stride + c * plane_stride
                    buf[o:o + pitch * hs].reshape(hs, pitch)[:, :ws] = f[c]
        else:
            pitch, plane_stride = 3 * ws + 5, 0
            frame_stride = pitch * hs + 7
            buf = np.full(n * frame_stride, 0x33, np.uint8)
            for i, f in enumerate(src):
                o = i * frame_stride
                buf[o:o + pitch * hs].reshape(hs, pitch)[:, :3 * ws] = f.reshape(hs, 3 * ws)
        d_src = torch.from_numpy(buf).cuda()
        gp, gs, lead = W + 3, (W + 3) * H + 9, 5
        d_gray = torch.full((lead + n * gs,), SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        eng.prepare_frames_layout_device(d_src.data_ptr(), pitch, frame_stride, plane_stride, ws, hs, 3, order, layout, n,
                                         d_gray.data_ptr() + lead, gp, gs)
        got = d_gray.cpu().numpy()
    inside = np.zeros(got.shape, bool)
    for i in range(n):
        o = lead + i * gs
        assert np.array_equal(got[o:o + gp * H].reshape(H, gp)[:, :W], want[i]), i
        inside[o:o + gp * H].reshape(H, gp)[:, :W] = True
    assert np.all(got[~inside] == SENT), "a byte outside the gray frames was written"


@pytest.mark.parametrize("algo", ["tvl1", "farn"])
@pytest.mark.parametrize("ws,hs", GEOMS)
def test_flows_of_rgb_channels_first_tensors(dfx, algo, ws, hs):
    import torch

    bgr = np.stack(_bgr(ws, hs))                       # (N, Hs, Ws, 3) B, G, R
    rgb_hwc = np.ascontiguousarray(bgr[..., ::-1])     # what a decoder hands out
    rgb_chw = np.ascontiguousarray(rgb_hwc.transpose(0, 3, 1, 2))
    with dfx.FlowEngine(W, H, algo, max_batch=MAX_BATCH) as eng:
        eng.set_source_format(ws, hs, 3)
        want = eng.flow_tensor(torch.from_numpy(bgr).cuda(), 1).cpu().numpy()
        eng.set_source_format(ws, hs, 3, order="rgb", layout="chw")
        # (N, 3, Hs, Ws) as the permuted view of an NHWC batch (torch's channels_last): read where it lies, interleaved
        nhwc = torch.from_numpy(rgb_hwc).cuda()
        got_perm = eng.flow_tensor(nhwc.permute(0, 3, 1, 2), 1).cpu().numpy()
        wide = torch.zeros((N_FRAMES, hs + 2, ws + 3, 3), dtype=torch.uint8, device="cuda")
        wide[:, 1:hs + 1, 2:ws + 2] = nhwc
        got_perm_padded = eng.flow_tensor(wide[:, 1:hs + 1, 2:ws + 2].permute(0, 3, 1, 2), 1).cpu().numpy()
        # an NCHW batch that is a permuted view of a planar-in-memory (N, Hs, 3, Ws) tensor: rows of the three planes interleave
        rows = torch.from_numpy(np.ascontiguousarray(rgb_chw.transpose(0, 2, 1, 3))).cuda()   # (N, Hs, 3, Ws)
        with pytest.raises(ValueError, match="overlap"):
            eng.flow_tensor(rows.permute(0, 2, 1, 3), 1)  # plane stride Ws < a plane: planes overlap
        # a non-contiguous view of a larger tensor: padded rows, planes and frames
        big = torch.zeros((N_FRAMES + 1, 4, hs + 3, ws + 9), dtype=torch.uint8, device="cuda")
        big[1:, 1:4, 2:hs + 2, 4:ws + 4] = torch.from_numpy(rgb_chw).cuda()
        view = big[1:, 1:4, 2:hs + 2, 4:ws + 4]
        assert not view.is_contiguous()
        got_view = eng.flow_tensor(view, 1).cpu().numpy()
        got_dense = eng.flow_tensor(torch.from_numpy(rgb_chw).cuda(), 1).cpu().numpy()
        got_host = eng.calc_optflows_planar(list(rgb_chw), 1)  # the host form: dense planes, 3 * Hs rows per frame
        # the same handle fed the BGR picture in the same layout: the order is really read
        bgr_chw = np.ascontiguousarray(bgr.transpose(0, 3, 1, 2))
        swapped = eng.flow_tensor(torch.from_numpy(bgr_chw).cuda(), 1).cpu().numpy()
        # RGB interleaved: the view of an NHWC batch as it lies in memory
        eng.set_source_format(ws, hs, 3, order="rgb")
        got_hwc = eng.flow_tensor(nhwc, 1).cpu().numpy()
        got_hwc_host = eng.calc_optflows_planar(list(rgb_hwc), 1)
    assert np.abs(want).max() > 0.1
    for name, got in [("view", got_view), ("dense", got_dense), ("host", got_host), ("hwc", got_hwc), ("hwc host", got_hwc_host),
                      ("permuted nhwc", got_perm), ("permuted padded nhwc", got_perm_padded)]:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert not np.array_equal(swapped, want), "an rgb handle fed BGR gave the BGR flows: the order is not read"


def test_set_size_restores_the_default_and_the_refusals(dfx):
    import torch

    ws, hs = 80, 44
    bgr = np.stack(_bgr(ws, hs))
    gray = SynthClip(W, H, 7).frames(N_FRAMES)

    def last_error(eng):
        return eng._L.dfx_last_error(eng._h).decode()

    with dfx.FlowEngine(W, H, "tvl1", max_batch=MAX_BATCH) as eng:
        want = eng.calc_optflows_planar(gray, 1)
        eng.set_source_format(ws, hs, 3, order="rgb", layout="chw")
        assert eng._frame_shape() == (3, hs, ws)
        with pytest.raises(ValueError):
            eng.flow_tensor(torch.from_numpy(np.stack(gray)).cuda(), 1)  # gray W x H frames no longer match
        eng.set_size(W, H)
        assert eng._frame_shape() == (H, W)
        assert np.array_equal(eng.flow_tensor(torch.from_numpy(np.stack(gray)).cuda(), 1).cpu().numpy(), want)
        # ValueError before the library
        for kw in (dict(order="gbr"), dict(layout="nchw"), dict(channels=1, order="rgb"), dict(channels=1, layout="chw")):
            args = dict(channels=3)
            args.update(kw)
            with pytest.raises(ValueError):
                eng.set_source_format(ws, hs, **args)
        # DFX_ERR_INVALID from the library, each with its text
        L, h = eng._L, eng._h
        for args, text in [((ws, hs, 3, 2, 0, 0), "order"), ((ws, hs, 3, 0, 2, 0), "order"), ((ws, hs, 3, -1, 0, 0), "order"),
                           ((ws, hs, 1, 1, 0, 0), "gray"), ((ws, hs, 1, 0, 1, 0), "gray"), ((ws, hs, 1, 0, 0, 64), "gray"),
                           ((ws, hs, 3, 1, 0, ws * hs), "plane_stride"), ((ws, hs, 3, 1, 1, ws * hs - 1), "plane_stride"),
                           ((ws, hs, 2, 0, 0, 0), "channels")]:
            assert L.dfx_set_source_format_ex(h, *args) == 1 and text in last_error(eng), args
        assert eng._frame_shape() == (H, W)  # the refused calls changed nothing
        assert np.array_equal(eng.calc_optflows_planar(gray, 1), want)
        # a plane stride below pitch * src_height is caught by the call that knows the pitch; host forms take dense planes
        d = torch.from_numpy(np.ascontiguousarray(bgr.transpose(0, 3, 1, 2))).cuda()
        out = torch.zeros((N_FRAMES - 1, 2, H, W), dtype=torch.float32, device="cuda")
        assert L.dfx_set_source_format_ex(h, ws, hs, 3, 1, 1, ws * hs + 8) == 0
        rc = L.dfx_calc_batch_planar_device(h, d.data_ptr(), ws + 1, 3 * (ws + 1) * hs + 64, N_FRAMES, 1, 0.0, out.data_ptr(), W,
                                            W * H, 2 * W * H)
        assert rc == 1 and "smaller than a frame" in last_error(eng)
        eng._src, eng._src_chw = (3, hs, ws), True  # (what set_source_format leaves; the plane stride was set beside it)
        with pytest.raises(dfx.DfxError) as e:
            eng.calc_optflows_planar(list(bgr.transpose(0, 3, 1, 2)), 1)
        assert e.value.status == 1 and "plane_stride" in last_error(eng)
        assert L.dfx_prepare_frames_layout_device(h, d.data_ptr(), ws, 3 * ws * hs, ws * hs - 1, ws, hs, 3, 1, 1, 1,
                                                  out.data_ptr(), W, W * H) == 1
        assert "smaller than a frame" in last_error(eng)
        assert L.dfx_prepare_frames_layout_device(h, d.data_ptr(), ws, 3 * ws * hs, 0, ws, hs, 3, 0, 3, 1, out.data_ptr(), W,
                                                  W * H) == 1
        assert "order" in last_error(eng)
        assert not bool(out.any()), "a refused call wrote"
