"""NumPy reference of the mask-aware flow median (dfx_flow_median_device; the arithmetic is stated in include/dfx.h).

Every sample is the unsigned key of its bit pattern, key(b) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000); the window is the
ksize x ksize positions with clamped coordinates; a sample is included where the mask is 0; the result is the included
sample of rank (m - 1) >> 1, or the input where m == 0.  The keys are sorted as 64-bit integers with the excluded samples at
2^32, above every key, so the reference does not share the device's 0xFFFFFFFF trick."""
import numpy as np

ALL, FILL = 0, 1  # DFX_MEDIAN_ALL / DFX_MEDIAN_FILL
MODES = {"all": ALL, "fill": FILL}


def key_of(bits):
    """The unsigned key of uint32 bit patterns."""
    bits = np.asarray(bits, np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def bits_of(key):
    """The inverse of key_of."""
    key = np.asarray(key, np.uint32)
    return key ^ np.where(key >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def _windows(plane, ksize):
    """(H, W, ksize * ksize) of an (H, W) plane, row-major over (dy, dx), coordinates clamped."""
    r = ksize // 2
    h, w = plane.shape
    p = np.pad(plane, r, mode="edge")
    return np.stack([p[j:j + h, i:i + w] for j in range(ksize) for i in range(ksize)], axis=-1)


def flow_median_ref(flow, ksize=5, mask=None, mode="all"):
    """One flow (2, H, W) float32 and an optional (H, W) uint8 mask -> (out (2, H, W) float32, mask_out (H, W) uint8 or
    None without a mask)."""
    flow = np.ascontiguousarray(flow, np.float32)
    assert flow.ndim == 3 and flow.shape[0] == 2 and ksize in (3, 5) and mode in MODES
    assert mask is not None or mode == "all"
    h, w = flow.shape[1:]
    excluded = np.zeros((h, w, ksize * ksize), bool) if mask is None else _windows(np.asarray(mask) != 0, ksize)
    m = (ksize * ksize - excluded.sum(-1)).astype(np.int64)
    rank = np.maximum(m - 1, 0) >> 1
    keep = m == 0
    if mode == "fill":
        keep = keep | (np.asarray(mask) == 0)
    out = np.empty_like(flow)
    for c in range(2):
        bits = flow[c].view(np.uint32)
        keys = _windows(key_of(bits), ksize).astype(np.uint64)
        keys[excluded] = np.uint64(1) << np.uint64(32)
        keys.sort(axis=-1)
        med = np.take_along_axis(keys, rank[..., None], axis=-1)[..., 0]
        med = bits_of(np.where(keep, 0, med).astype(np.uint32))
        out[c] = np.where(keep, bits, med).view(np.float32)
    return out, (None if mask is None else (m == 0).astype(np.uint8))


def flow_median_batch(flows, ksize=5, masks=None, mode="all", passes=1):
    """(M, 2, H, W) flows and optional (M, H, W) masks through `passes` applications, mask_out fed back as the mask; in
    fill mode the passes stop once a returned mask is all zero, as FlowEngine.flow_median does."""
    flows = np.asarray(flows, np.float32)
    for k in range(passes):
        res = [flow_median_ref(flows[i], ksize, None if masks is None else masks[i], mode) for i in range(len(flows))]
        flows = np.stack([r[0] for r in res]) if res else flows
        if masks is not None:
            masks = np.stack([r[1] for r in res]) if res else masks
            if mode == "fill" and not masks.any():
                break
    return flows, masks


def special_field():
    """A 6 x 7 flow whose windows hold -0 / +0, both infinities, NaNs of both signs with payloads, and subnormals, as bit
    patterns: u row-major from this table, v the table reversed."""
    nan_pos, nan_neg = 0x7FC00001, 0xFFC00002     # quiet NaNs with payloads
    snan_pos, snan_neg = 0x7F800001, 0xFF800001   # signalling NaNs
    top = 0x7FFFFFFF                              # the NaN whose key is 0xFFFFFFFF
    sub_pos, sub_neg = 0x00000001, 0x80000001     # the smallest subnormals
    one, mone = 0x3F800000, 0xBF800000
    table = [0x00000000, 0x80000000, one, mone, 0x7F800000, 0xFF800000, nan_pos,
             nan_neg, sub_pos, sub_neg, 0x007FFFFF, 0x807FFFFF, snan_pos, snan_neg,
             top, 0x00800000, 0x80800000, 0x40000000, 0xC0000000, 0x00000000, 0x80000000,
             one, one, mone, mone, sub_pos, sub_pos, sub_neg,
             0x7F7FFFFF, 0xFF7FFFFF, nan_pos, nan_neg, 0x80000000, 0x00000000, top,
             0x3F000000, 0xBF000000, 0x7F800000, 0xFF800000, 0xFFFFFFFF, snan_pos, 0x00000000]
    u = np.array(table, np.uint32).reshape(6, 7)
    return np.stack([u, u[::-1, ::-1]]).view(np.float32)


def blob_mask(rng, h, w, share=0.3):
    """A thresholded smooth field: the shape an occlusion mask has."""
    f = rng.standard_normal((h + 8, w + 8))
    k = np.ones(5) / 5.0
    for axis in (0, 1):
        f = np.apply_along_axis(lambda a: np.convolve(a, k, mode="same"), axis, f)
    f = f[4:4 + h, 4:4 + w]
    return (f > np.quantile(f, 1.0 - share)).astype(np.uint8) if f.size > 1 else np.zeros((h, w), np.uint8)
