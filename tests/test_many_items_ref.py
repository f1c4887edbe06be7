"""The discrimination check of tests/test_many_items_gpu.py on reference output alone (no GPU): the 7 base items of a batch of
more than 65535 give pairwise different reference items in every output that is compared, so that an item taken from one
place further on or back is a mismatch; item 5 holds the NaN and the masked pixel; the mask and validity planes are not
constant."""
import os
import re

import numpy as np
import pytest

from tests import many_items_cases as M


@pytest.mark.parametrize("op", sorted(M.REFERENCES))
def test_the_reference_items_are_pairwise_different(op):
    ref = M.check_distinct(op)
    for name, a in ref.items():
        assert len(a) in (M.K, M.K + 1, M.K + 2), (op, name)
        assert not a.flags.writeable


def test_the_base_items():
    b = M.base()
    for name, a in b.items():
        if name != "last":
            M.distinct(("base", name), a)
    assert np.isnan(b["flows"][5]).sum() == 1 and b["masks"][5].any() and not np.isnan(np.delete(b["flows"], 5, 0)).any()
    assert all(0 < (m != 0).sum() < m.size for m in b["masks"]), "a mask plane is constant"
    for op in M.REFERENCES:  # the phase shifts at every launch boundary
        assert M.chunk(op) % M.period(op) == 1 and M.period(op) > 5, op
    assert M.chunk("interpolate") == 32767 and M.chunk("warp") == 65535 and (M.GRID_MAX // 2) % M.K == 0
    assert M.counts(M.GRID_MAX) == [65535, 65536, 131071] and M.counts(M.GRID_MAX // 2) == [32767, 32768, 65535]


def test_the_bound_of_a_launch_is_named_once():
    """DFX_GRID_YZ_MAX is what the tests take for it, and no launcher writes the number out."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "denseflow_amd", "csrc")
    with open(os.path.join(csrc, "dfx_device.h")) as f:
        assert re.search(r"constexpr int DFX_GRID_YZ_MAX = (\d+);", f.read()).group(1) == str(M.GRID_MAX)
    with open(os.path.join(csrc, "flow_quad.h")) as f:
        assert "constexpr int FQ_ITEMS_MAX = DFX_GRID_YZ_MAX;" in f.read()
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".hip"):
            with open(os.path.join(csrc, name)) as f:
                code = re.sub(r"//[^\n]*", "", f.read())
            assert not re.search(r"\b(65535|32767)\b", code), name


def test_the_planes_that_say_where_are_not_constant():
    for op, names in (("fb_check", ("occ",)), ("warp", ("valid",)), ("flow_chain", ("all_valid", "last_valid")),
                      ("flow_median", ("mask_out",)), ("global_motion", ("moving",)), ("flow_project", ("hole",)),
                      ("splat", ("hole",)), ("interpolate", ("source",))):
        ref = M.REFERENCES[op]()
        for name in names:
            assert len(np.unique(ref[name])) > 1, (op, name)
