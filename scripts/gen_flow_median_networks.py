#!/usr/bin/env python3
"""Writes denseflow_amd/csrc/flow_median_networks.h: the compare-exchange networks of the flow median kernels
(flow_median_kernels.hip) as macro lists, and proves each with the 0-1 principle over all 2^n inputs before it writes.

  FM_NET9_MEDIAN / FM_NET25_MEDIAN   fixed-rank selection: wire 4 / 12 ends as the median (19 and 99 exchanges, the
                                     networks of cv::medianBlur's CV_32F path as oracle/cpu_tvl1_baseline.c restates them)
  FM_NET9_LOW5 / FM_NET25_LOW13      wires 0 .. 4 / 0 .. 12 end as the 5 / 13 smallest in ascending order: Batcher's
                                     odd-even merge sort of 16 / 32 wires, the wires past n holding the largest key (an
                                     exchange with one is the identity and is dropped), then pruned backwards to the exchanges
                                     the wanted outputs depend on

X(a, b) leaves min on wire a and max on wire b; a > b occurs in the 9-median.  Usage: python scripts/gen_flow_median_networks.py
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "denseflow_amd", "csrc", "flow_median_networks.h")

MED9 = [(1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 3), (5, 8), (4, 7), (3, 6), (1, 4), (2, 5),
        (4, 7), (4, 2), (6, 4), (4, 2)]
MED25 = [(0, 1), (3, 4), (2, 4), (2, 3), (6, 7), (5, 7), (5, 6), (9, 10), (8, 10), (8, 9), (12, 13), (11, 13), (11, 12),
         (15, 16), (14, 16), (14, 15), (18, 19), (17, 19), (17, 18), (21, 22), (20, 22), (20, 21), (23, 24), (2, 5), (3, 6),
         (0, 6), (0, 3), (4, 7), (1, 7), (1, 4), (11, 14), (8, 14), (8, 11), (12, 15), (9, 15), (9, 12), (13, 16), (10, 16),
         (10, 13), (20, 23), (17, 23), (17, 20), (21, 24), (18, 24), (18, 21), (19, 22), (8, 17), (9, 18), (0, 18), (0, 9),
         (10, 19), (1, 19), (1, 10), (11, 20), (2, 20), (2, 11), (12, 21), (3, 21), (3, 12), (13, 22), (4, 22), (4, 13),
         (14, 23), (5, 23), (5, 14), (15, 24), (6, 24), (6, 15), (7, 16), (7, 19), (13, 21), (15, 23), (7, 13), (7, 15), (1, 9),
         (3, 11), (5, 17), (11, 17), (9, 17), (4, 10), (6, 12), (7, 14), (4, 6), (4, 7), (12, 14), (10, 14), (6, 7), (10, 12),
         (6, 10), (6, 17), (12, 17), (7, 17), (7, 10), (12, 18), (7, 12), (10, 18), (12, 20), (10, 20), (10, 12)]


def batcher(n):
    """Batcher's odd-even merge sort of n = 2^k wires."""
    net, p = [], 1
    while p < n:
        k = p
        while k >= 1:
            for j in range(k % p, n - k, 2 * k):
                for i in range(min(k, n - j - k)):
                    if (i + j) // (2 * p) == (i + j + k) // (2 * p):
                        net.append((i + j, i + j + k))
            k //= 2
        p *= 2
    return net


def low(n, keep):
    """The exchanges of a sort of n wires that wires 0 .. keep-1 depend on."""
    size = 1
    while size < n:
        size *= 2
    net = [(a, b) for a, b in batcher(size) if a < n and b < n]
    live, kept = set(range(keep)), []
    for a, b in reversed(net):
        if a in live or b in live:
            kept.append((a, b))
            live |= {a, b}
    return kept[::-1]


def run01(net, n):
    """Wire values after the network for every 0-1 input: bit x of wire i starts as bit i of x."""
    x = np.arange(1 << n, dtype=np.uint32)
    wires = [np.packbits(((x >> i) & 1).astype(np.uint8)) for i in range(n)]
    for a, b in net:
        wires[a], wires[b] = wires[a] & wires[b], wires[a] | wires[b]
    ones = np.zeros(1 << n, np.uint8)
    for i in range(n):
        ones += ((x >> i) & 1).astype(np.uint8)
    return wires, ones


def prove(net, n, outputs):
    """Wire j of `outputs` ends as the sample of rank j: for a 0-1 input with z zeros that is 1 exactly where j >= z."""
    wires, ones = run01(net, n)
    for j in outputs:
        want = np.packbits((ones >= n - j).astype(np.uint8))
        assert np.array_equal(wires[j], want), (n, j)


def macro(name, net):
    body, line = [], "#define " + name + "(X)"
    for a, b in net:
        item = f" X({a}, {b})"
        if len(line) + len(item) > 122:
            body.append(line + " \\")
            line = "   "
        line += item
    return "\n".join(body + [line])


def main():
    low5, low13 = low(9, 5), low(25, 13)
    prove(MED9, 9, [4])
    prove(MED25, 25, [12])
    prove(low5, 9, range(5))
    prove(low13, 25, range(13))
    text = f"""// flow_median_networks.h — written by scripts/gen_flow_median_networks.py, which proves every list with the 0-1 principle
// over all 2^n inputs before it writes; do not edit.  X(a, b) is a compare-exchange: min to wire a, max to wire b.
//   FM_NET9_MEDIAN   {len(MED9)} exchanges: wire 4 ends as the median of 9
//   FM_NET25_MEDIAN  {len(MED25)} exchanges: wire 12 ends as the median of 25
//   FM_NET9_LOW5     {len(low5)} exchanges: wires 0 .. 4 end as the 5 smallest of 9, ascending
//   FM_NET25_LOW13   {len(low13)} exchanges: wires 0 .. 12 end as the 13 smallest of 25, ascending
#pragma once

{macro("FM_NET9_MEDIAN", MED9)}

{macro("FM_NET25_MEDIAN", MED25)}

{macro("FM_NET9_LOW5", low5)}

{macro("FM_NET25_LOW13", low13)}
"""
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: median 9 / 25 in {len(MED9)} / {len(MED25)} exchanges, low 5 of 9 / low 13 of 25 in {len(low5)} / {len(low13)}")


if __name__ == "__main__":
    main()
