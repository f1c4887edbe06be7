"""Row segments of the Farneback row-stream iteration kernel for every window it is built for (farn_stream_seg_rows,
denseflow_amd/csrc/farneback_plan.h; no GPU): the segments partition [0, h), their length is whole 6-row steps, and no
segment is shorter than four times the 2 * half warm-up rows it recomputes unless the level itself is."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HALVES = range(3, 11)  # winSize 7 .. 21


@pytest.fixture(scope="module")
def plan():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libfarn_stream_plan.%d.so" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                    os.path.join(HERE, "farn_stream_plan_harness.cpp")], check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)
    return L


def test_the_kernel_is_built_for_windows_7_to_21(plan):
    assert [half for half in range(0, 17) if plan.fsp_has_half(half)] == list(HALVES)


@pytest.mark.parametrize("half", HALVES)
def test_the_floor_follows_the_warm_up_rows(plan, half):
    step = plan.fsp_step_rows()
    floor = plan.fsp_min_seg_rows(half)
    assert step == 6 and floor % step == 0
    assert 4 * 2 * half <= floor < 4 * 2 * half + step  # four times the warm-up rows, rounded up to whole steps
    if half == 6:
        assert floor == 48  # the reference's window: the value the kernel was tuned with


@pytest.mark.parametrize("half", HALVES)
def test_segments_partition_the_rows(plan, half):
    floor = plan.fsp_min_seg_rows(half)
    heights = sorted({1, 5, 6, 7, 2 * half, floor - 1, floor, floor + 1, 2 * floor - 1, 2 * floor, 2 * floor + 1, 77, 270, 500,
                      1080, 2160, 8192})
    for h in heights:
        for w in (1, 64, 65, 480, 1920, 8192):
            for n_pairs in (1, 2, 129, 2048):
                rows = plan.fsp_seg_rows(w, h, n_pairs, half)
                assert rows > 0 and rows % 6 == 0, (w, h, n_pairs)
                nseg = -(-h // rows)
                assert (nseg - 1) * rows < h <= nseg * rows, (w, h, n_pairs)  # a partition, the last segment not empty
                if nseg > 1:  # a level is cut only into segments of at least the floor (h < floor: one segment)
                    assert rows >= floor, (w, h, n_pairs, rows)
                    assert h >= 2 * floor or rows * (nseg - 1) >= floor
                if h < 2 * floor:
                    assert nseg == 1, (w, h, n_pairs)


def test_many_small_launches_are_cut_down_to_the_floor(plan):
    """One pair of one strip: the plan wants 16 generations of workgroups, so the segments are as short as the floor allows."""
    for half in HALVES:
        floor = plan.fsp_min_seg_rows(half)
        h = 40 * floor
        rows = plan.fsp_seg_rows(64, h, 1, half)
        assert rows == floor, (half, rows)


def test_the_default_is_the_reference_window(plan):
    for w, h, n in [(1920, 1080, 129), (70, 500, 2), (1000, 77, 2), (33, 40, 1), (8192, 8192, 1)]:
        assert plan.fsp_seg_rows_default(w, h, n) == plan.fsp_seg_rows(w, h, n, 6)
