"""CPU test of the engines' out-of-memory rules (denseflow_amd/csrc/engine_buffers.h, the header every *_engine.cpp grows
its buffers through): what a failed allocation leaves of a grow-only buffer, of a device + pinned table and of TVL1's
per-pair tables, what batch set_size then goes on with, and how many frame slots an engine may count afterwards.  No test
on the device reaches these paths.  tests/engine_buffers_harness.cpp holds the cases and an allocator that fails on
command; every case checks exact values and ends with nothing allocated."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [
    "grow_large_enough_is_untouched",
    "grow_frees_the_old_buffer_first",
    "grow_failure_restores_the_old_size",
    "grow_failure_without_restore_leaves_nothing",
    "table_grow_succeeds",
    "table_device_failure_keeps_the_old_pair",
    "table_pinned_failure_keeps_the_old_pair",
    "per_pair_tables_grow_all_or_nothing",
    "fit_halves_the_batch_until_it_fits",
    "fit_falls_back_to_the_held_allocation",
    "fit_fails_when_not_one_slot_is_held",
    "fit_reports_batch_0_exactly_when_nothing_came_back",
    "slot_rule_three_equal_buffers_ensure",
    "slot_rule_three_equal_buffers_set_size",
    "slot_rule_four_unequal_buffers_ensure",
    "slot_rule_four_unequal_buffers_set_size",
    "slot_rule_without_the_conditional_buffer",
    "slot_rule_counts_nothing_new_on_failure",
]


@pytest.fixture(scope="module")
def eb():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libengine_buffers_harness.%d.so" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "engine_buffers_harness.cpp")],
                   check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)
    L.eb_case_name.restype = C.c_char_p
    L.eb_run.argtypes = [C.c_int, C.c_char_p, C.c_int]
    return L


def test_every_case_of_the_harness_is_run(eb):
    assert [eb.eb_case_name(i).decode() for i in range(eb.eb_case_count())] == CASES


@pytest.mark.parametrize("name", CASES)
def test_case(eb, name):
    msg = C.create_string_buffer(512)
    rc = eb.eb_run(CASES.index(name), msg, len(msg))
    assert rc == 0, msg.value.decode()


def test_the_header_needs_no_hip():
    """engine_buffers.h is host logic behind an allocator policy: plain g++ compiles it (the fixture above has), and neither
    it nor the headers it includes name a HIP header."""
    csrc = os.path.join(HERE, "..", "denseflow_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-M", "-x", "c++", os.path.join(csrc, "engine_buffers.h")],
                       check=True, capture_output=True, text=True)
    assert "engine_plan.h" in r.stdout and "hip_runtime" not in r.stdout and "/hip/" not in r.stdout
