"""Mints tests/golden/jpeg_colour_golden.npz: libjpeg-turbo's files (through Pillow) for the seeded colour frames of
tests/colour_cases.py, for the boxes without Pillow.  Run from the repository root: python tests/golden/make_jpeg_colour_golden.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import colour_cases as cc  # noqa: E402

if __name__ == "__main__":
    out = {}
    for kind, w, h, q in cc.GOLDEN_CASES:
        out[cc.golden_key(kind, w, h, q)] = np.frombuffer(cc.libjpeg(cc.frame(kind, w, h, 0), q), np.uint8)
    np.savez_compressed(cc.GOLDEN, **out)
    print(len(out), "files,", os.path.getsize(cc.GOLDEN), "bytes")
