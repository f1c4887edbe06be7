"""Mint tests/golden/ref_fresh_golden.npz: what THE REFERENCE'S OWN LINES return on the "fresh" inputs of
tests/test_oracle_quant.py — convertFlowToImage (oracle/_ref/libref_quant.so) on adversarial flows under six bound pairs,
convertFlowToPngImage (oracle/_ref/libref_png.so) on twelve flows of random sizes and extrema — so that those tests hold the
oracle against the reference where the reference tree is absent too (they compare with the live libraries as well when
`make -C oracle ref` has built them).  The inputs are regenerated from their seeds; only the outputs are stored.
Needs the reference tree.  Usage:  python tests/golden/make_ref_fresh_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import oracle_py as O  # noqa: E402
from tests.golden.make_png_planes_golden import flow_with_extrema  # noqa: E402
from tests.golden.make_quant_golden import adversarial_flow  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "ref_fresh_golden.npz")

QUANT_BOUNDS = [(-20, 20), (-32, 32), (-1, 1), (-5, 20), (0, 0), (3, -3)]


def quant_fresh_flows():
    """[(lo, hi, flow)]: an 80x50 adversarial flow per bound pair, seeds 100, 101, ..."""
    return [(lo, hi, adversarial_flow(max(abs(hi), 1), 80, 50, 100 + seed)) for seed, (lo, hi) in enumerate(QUANT_BOUNDS)]


def png_fresh_flows():
    """[(w, h, k, flow)]: twelve flows of random sizes and extrema (seed 3), the signs of the extrema alternating."""
    rng = np.random.default_rng(3)
    out = []
    for k in range(12):
        w, h = int(rng.integers(1, 90)), int(rng.integers(1, 70))
        flow = flow_with_extrema(w, h, float(rng.choice([0.0, 0.3, 7.9, 15.5, 31.7, 300.0])),
                                 float(rng.choice([0.0, 1.0, 3.9, 23.6, 64.0])), 200 + k, bool(k & 1))
        out.append((w, h, k, flow))
    return out


def main():
    O.build()
    assert O.ref_quant_available() and O.ref_png_available(), "oracle/_ref missing (needs the reference tree)"
    out = {}
    for i, (lo, hi, flow) in enumerate(quant_fresh_flows()):
        out[f"quant_{i}_x"], out[f"quant_{i}_y"] = O.ref_flow_to_u8(flow, lo, hi)
    for w, h, k, flow in png_fresh_flows():
        out[f"png_{k}_bgr"] = O.ref_flow_to_png_image(flow)
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, len(out), "arrays")


if __name__ == "__main__":
    main()
