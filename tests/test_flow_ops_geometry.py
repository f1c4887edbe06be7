"""The one home of the stride rules of the calls on finished flows (fb_check .. flow_colour): _flow_geometry for
(n, 2, H, W) float32 flows, _plane_geometry for (n, H, W) masks and weights.  CPU tensors, no library: the helpers read
shape and strides only.  Every expected tuple is written out from the rules — a dimension of extent 1 takes its stride
from the dense layout, not from the tensor."""
import pytest
import torch

from denseflow_amd.engine import _flow_geometry, _plane_geometry

SIZES = [(1, 1), (5, 1), (1, 4), (9, 6)]  # (W, H)
ITEMS = [1, 3]
PAD = 3


def flows(n, H, W):
    return torch.zeros((n, 2, H, W), dtype=torch.float32)


@pytest.mark.parametrize("n", ITEMS)
@pytest.mark.parametrize("W,H", SIZES)
def test_flow_geometry_accepts(W, H, n):
    # contiguous
    assert _flow_geometry(flows(n, H, W), H, W, "flows") == (W, H * W, 2 * H * W)
    # rows padded: the pitch is the tensor's only where there is a second row
    t = flows(n, H, W + PAD)[..., :W]
    assert _flow_geometry(t, H, W, "flows") == (W + PAD if H > 1 else W, H * (W + PAD), 2 * H * (W + PAD))
    # planes padded
    t = flows(n, H + 2, W)[:, :, :H]
    assert _flow_geometry(t, H, W, "flows") == (W, (H + 2) * W, 2 * (H + 2) * W)
    # every second flow of a batch: the flow stride is the tensor's only where there is a second flow
    t = flows(2 * n, H, W)[::2]
    assert t.shape[0] == n
    assert _flow_geometry(t, H, W, "flows") == (W, H * W, 4 * H * W if n > 1 else 2 * H * W)


@pytest.mark.parametrize("n", ITEMS)
@pytest.mark.parametrize("W,H", SIZES)
def test_flow_geometry_refuses(W, H, n):
    words = "flows: the innermost dimension must be contiguous and rows, planes and flows must not overlap"
    if n > 1:  # one flow repeated: flow stride 0
        with pytest.raises(ValueError, match=words):
            _flow_geometry(flows(1, H, W).expand(n, 2, H, W), H, W, "flows")
    t = flows(n, H, 2 * W)[..., ::2]  # pixel stride 2
    if W > 1:
        with pytest.raises(ValueError, match=words):
            _flow_geometry(t, H, W, "flows")
    else:  # one pixel per row: its stride is never used
        assert _flow_geometry(t, H, W, "flows") == (2 if H > 1 else 1, 2 * H, 4 * H)
    with pytest.raises(ValueError, match=r"flows must be an \(M, 2, H, W\) torch.float32 tensor$"):
        _flow_geometry(flows(n, H, W).double(), H, W, "flows")
    t = torch.zeros((n, H, W, 2), dtype=torch.float32).permute(0, 3, 1, 2)  # interleaved (u, v) pixels
    if (W, H) == (1, 1):  # one pixel: interleaved and planar are the same two floats
        assert _flow_geometry(t, H, W, "flows") == (1, 1, 2)
    else:
        with pytest.raises(ValueError, match=words):
            _flow_geometry(t, H, W, "flows")


def test_flow_geometry_words():
    H, W = 6, 9
    with pytest.raises(ValueError, match=r"^out must be an \(N, 2, H, W\) torch.float32 tensor$"):
        _flow_geometry(flows(2, H, W + 1), H, W, "out", "N")
    with pytest.raises(ValueError, match=r"^fwd must be an \(n, 2, H, W\) torch.float32 tensor, one flow per pair$"):
        _flow_geometry(flows(2, H, W), H, W, "fwd", "n", 3, ", one flow per pair")
    assert _flow_geometry(flows(3, H, W), H, W, "fwd", "n", 3, ", one flow per pair") == (W, H * W, 2 * H * W)
    for bad in (None, flows(2, H, W).numpy(), flows(2, H, W)[0]):
        with pytest.raises(ValueError, match="flows must be an"):
            _flow_geometry(bad, H, W, "flows")
    with pytest.raises(ValueError, match="^out: the innermost"):
        _flow_geometry(flows(2, H, 2 * W)[..., ::2], H, W, "out")


def planes(n, H, W, dtype=torch.uint8):
    return torch.zeros((n, H, W), dtype=dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("n", ITEMS)
@pytest.mark.parametrize("W,H", SIZES)
def test_plane_geometry_accepts(W, H, n, dtype):
    assert _plane_geometry(planes(n, H, W, dtype), n, H, W, dtype, "mask") == (W, H * W)
    # rows padded: pitch and stride are the tensor's only where there is a second row / a second plane
    t = planes(n, H, W + PAD, dtype)[..., :W]
    pitch = W + PAD if H > 1 else W
    assert _plane_geometry(t, n, H, W, dtype, "mask") == (pitch, H * (W + PAD) if n > 1 else H * pitch)
    # planes padded
    t = planes(n, H + 2, W, dtype)[:, :H]
    assert _plane_geometry(t, n, H, W, dtype, "mask") == (W, (H + 2) * W if n > 1 else H * W)
    # every second plane of a batch
    t = planes(2 * n, H, W, dtype)[::2]
    assert _plane_geometry(t, n, H, W, dtype, "mask") == (W, 2 * H * W if n > 1 else H * W)


@pytest.mark.parametrize("n", ITEMS)
@pytest.mark.parametrize("W,H", SIZES)
def test_plane_geometry_refuses(W, H, n):
    words = "mask: the innermost dimension must be contiguous and rows and masks must not overlap"
    if n > 1:  # one plane repeated: stride 0
        with pytest.raises(ValueError, match=words):
            _plane_geometry(planes(1, H, W).expand(n, H, W), n, H, W, torch.uint8, "mask")
    t = planes(n, H, 2 * W)[..., ::2]  # pixel stride 2
    if W > 1:
        with pytest.raises(ValueError, match=words):
            _plane_geometry(t, n, H, W, torch.uint8, "mask")
    else:  # one pixel per row: its stride is never used
        pitch = 2 if H > 1 else 1
        assert _plane_geometry(t, n, H, W, torch.uint8, "mask") == (pitch, 2 * H if n > 1 else H * pitch)
    with pytest.raises(ValueError, match=r"^mask must be an \(M, H, W\) torch.uint8 tensor$"):
        _plane_geometry(planes(n, H, W, torch.float32), n, H, W, torch.uint8, "mask")
    t = torch.zeros((H, W, n), dtype=torch.uint8).permute(2, 0, 1)  # the n planes interleaved pixel by pixel
    if n == 1:  # a single plane: dense
        assert _plane_geometry(t, n, H, W, torch.uint8, "mask") == (W, H * W)
    elif (W, H) == (1, 1):  # one pixel per plane, one byte apart
        assert _plane_geometry(t, n, H, W, torch.uint8, "mask") == (1, 1)
    else:
        with pytest.raises(ValueError, match=words):
            _plane_geometry(t, n, H, W, torch.uint8, "mask")


def test_plane_geometry_words():
    H, W = 6, 9
    with pytest.raises(ValueError, match=r"^importance must be an \(N, H, W\) torch.float32 tensor$"):
        _plane_geometry(planes(2, H, W), 2, H, W, torch.float32, "importance", "N", "planes")
    with pytest.raises(ValueError, match="^importance: the innermost dimension must be contiguous and rows and planes must not overlap$"):
        _plane_geometry(planes(2, H, 2 * W, torch.float32)[..., ::2], 2, H, W, torch.float32, "importance", "N", "planes")
    with pytest.raises(ValueError, match=r"^occ must be an \(n, H, W\) torch.uint8 tensor$"):
        _plane_geometry(planes(3, H, W), 2, H, W, torch.uint8, "occ", "n")  # one plane per flow
    with pytest.raises(ValueError, match="occ must be an"):
        _plane_geometry(None, 2, H, W, torch.uint8, "occ")
