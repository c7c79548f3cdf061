"""The two kernels of svp_shortcut.hip (a module of their own): they exist in the built code objects, spill no vector and
no scalar register, have no private segment, and match profiles/svp_shortcut_kernel_resources.txt.  Their names keep clear
of the substrings the other resource tests select by -- the kernels with `svp_` in their name are still the seven of
svp_space.hip -- and the walk and the search are shared, not restated.  Read from the built code objects
(tools/kernel_resources.py).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ["rkh::rl1cut_pairs_kernel", "rkh::rl1cut_time_in_kernel"]
RESERVED = ("svp_", "rl1rrt_", "nn1_", "kinematics", "records", "depth", "propagate_pair", "propagate_kernel<6",
            "edge_points_kernel<6", "edge_check_kernel", "shortcut")


@pytest.fixture(scope="module")
def res():
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    return kr.kernel_resources()


def _table(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        if line.startswith("#") or line.startswith("kernel") or not line.strip():
            continue
        rows[line[:78].strip()] = [int(x) for x in line[78:].split()]
    return rows


def test_the_two_kernels_exist_match_the_table_and_spill_nothing(res):
    table = _table("svp_shortcut_kernel_resources.txt")
    built = {k for k in res if "rl1cut_" in k}
    assert built == set(KERNELS) == set(table), built ^ set(KERNELS)
    for k in KERNELS:
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "lds", d["group_segment_fixed_size"])
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert d["private_segment_fixed_size"] == 0 and d["group_segment_fixed_size"] == 0, (k, d)
        assert d["vgpr_count"] <= 64 and d["agpr_count"] == 0, (k, d)   # eight waves per SIMD: they only move memory
        assert d["max_flat_workgroup_size"] == 256, (k, d)
        assert table[k][:6] == [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"],
                                d["private_segment_fixed_size"], d["group_segment_fixed_size"]], (k, table[k], d)


def test_kernel_names_keep_clear_of_the_reserved_substrings(res):
    for k in KERNELS:
        assert not [s for s in RESERVED if s in k], k
    assert len([k for k in res if "svp_" in k]) == 7
    # the search is path_shortcut.hip's: the kernels with `shortcut` in their name are still its two
    assert sorted(k for k in res if "shortcut" in k) == ["rkh::shortcut_dp_kernel", "rkh::shortcut_pairs_kernel"]


def test_the_walk_and_the_search_are_shared_not_restated():
    text = open(os.path.join(ROOT, "reak_amd", "csrc", "svp_shortcut.hip")).read()
    assert "launch_svp_walk(" in text and "svp_walk_points_kernel" not in text and "svp_walk_layout(" in text
    assert "launch_shortcut_dp(" in text and "shortcut_dp_kernel(" not in text
    assert '#include "path_shortcut.h"' in text and "shortcut_pair_at(" in text and "shortcut_pair_index(" in text
    make = open(os.path.join(ROOT, "reak_amd", "csrc", "Makefile")).read()
    assert "svp_shortcut.hip" in make.split("OBJ =")[0]
    assert "svp_shortcut.o: path_shortcut.h svp_device.h" in make
