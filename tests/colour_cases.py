"""Shared by the colour -s=0 tests and by tests/golden/make_jpeg_colour_golden.py: the sizes, qualities and seeded frame
contents of the colour JPEG pin, the libjpeg-turbo reference (through Pillow) and the golden file's keys."""
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_colour_golden.npz")

# ceil(W/8) and ceil(H/8) odd and even independently (dummy blocks right, bottom, both, none), odd widths / heights (edge
# replication before downsampling), sub-MCU images
SIZES = [(1, 1), (5, 3), (8, 8), (16, 16), (17, 9), (24, 16), (16, 24), (33, 17), (70, 45), (257, 131), (640, 360),
         (1920, 1080)]
QUALITIES = (1, 10, 50, 75, 90, 95, 100)
KINDS = ("smooth", "noise", "primaries", "constant")


def qualities(w, h):
    return (95, 50) if w * h > 500000 else QUALITIES


def frame(kind, w, h, seed):
    """A seeded (h, w, 3) uint8 BGR frame."""
    rng = np.random.default_rng([seed, w, h, KINDS.index(kind)])
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "smooth":
        ch = [128 + 90 * np.sin(xx / (9.0 + 2 * c)) * np.cos(yy / (5.0 + c)) + rng.normal(0, 6, (h, w)) for c in range(3)]
        return np.ascontiguousarray(np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8))
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "primaries":  # pure R / G / B / white / black patches: the colour-conversion extremes
        palette = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [255, 255, 255], [0, 0, 0]], np.uint8)  # BGR
        idx = ((xx // 5) + 2 * (yy // 3) + seed) % 5
        return np.ascontiguousarray(palette[idx])
    return np.full((h, w, 3), rng.integers(0, 256, 3), np.uint8)


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


def libjpeg(bgr, quality):
    """libjpeg-turbo's file for a BGR frame, as cv::imencode(".jpg", bgr) drives it (through Pillow)."""
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]), "RGB").save(b, "JPEG", quality=quality)
    return b.getvalue()


def golden_key(kind, w, h, q):
    return f"{kind}_{w}x{h}_q{q}"


# what the golden file holds (small enough to commit): every size below 1080p at three qualities, two kinds
GOLDEN_CASES = [(kind, w, h, q) for (w, h) in SIZES if w * h <= 640 * 360 for q in (10, 75, 95)
                for kind in ("smooth", "primaries") if w * h <= 70 * 45 or (q == 95 and kind == "smooth" and w < 640)]

_golden = None


def golden(kind, w, h, q):
    """libjpeg-turbo's bytes from the committed golden file, or None when the case is not in it."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN)) if os.path.exists(GOLDEN) else {}
    v = _golden.get(golden_key(kind, w, h, q))
    return None if v is None else v.tobytes()


def reference(kind, w, h, q, bgr):
    """(bytes, source) for a case: Pillow live where it imports, else the golden file; (None, None) when neither has it."""
    if have_pillow():
        return libjpeg(bgr, q), "pillow"
    g = golden(kind, w, h, q)
    return (g, "golden") if g is not None else (None, None)


def segments(data):
    """Marker bytes of a JPEG file's segments up to and including SOS, and their payloads."""
    out, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while i < len(data):
        assert data[i] == 0xFF
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        out.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            break
    return out
