"""The kernels of svp_planner.hip (a module of their own): they exist in the built code objects, spill no vector and no
scalar register, have no private segment, and match profiles/r22_svp_rrt_kernel_resources.txt.  Their names keep clear of
`svp_` -- tests/test_svp_space_resources.py holds the set of kernels with that substring to the seven of svp_space.hip --
and of the substrings tests/test_kernel_resources.py selects by.  Read from the built code objects
(tools/kernel_resources.py).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ["rkh::rl1rrt_init_kernel", "rkh::rl1rrt_sample_kernel", "rkh::rl1rrt_nearest_kernel", "rkh::rl1rrt_steer_kernel",
           "rkh::rl1rrt_commit_kernel", "rkh::rl1rrt_finish_kernel"]
RESERVED = ("svp_", "nn1_", "propagate_pair", "propagate_kernel<6", "edge_points_kernel<6", "edge_check_kernel")


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


def test_planner_kernels_exist_match_the_table_and_spill_nothing(res):
    table = _table("r22_svp_rrt_kernel_resources.txt")
    built = {k for k in res if "rl1rrt_" in k}
    assert built == set(KERNELS) == set(table), built ^ set(KERNELS)
    for k in KERNELS:
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "lds", d["group_segment_fixed_size"])
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert d["private_segment_fixed_size"] == 0, (k, d)
        assert d["vgpr_count"] <= 128 and d["agpr_count"] == 0, (k, d)   # four waves per SIMD at the least
        assert d["max_flat_workgroup_size"] == 256, (k, d)
        assert table[k][:6] == [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"],
                                d["private_segment_fixed_size"], d["group_segment_fixed_size"]], (k, table[k], d)
    # the sample kernel's LDS is the generator's 624 words and one more; the nearest kernel's the query and the reduction
    assert res["rkh::rl1rrt_sample_kernel"]["group_segment_fixed_size"] == 625 * 4
    assert res["rkh::rl1rrt_nearest_kernel"]["group_segment_fixed_size"] == 24 * 8 + 4 * 8 + 4 * 4


def test_planner_kernel_names_keep_clear_of_the_reserved_substrings(res):
    for k in KERNELS:
        assert not [s for s in RESERVED if s in k], k
    # the walk the planner launches is svp_space.hip's: the kernels with `svp_` in their name are still its seven
    assert len([k for k in res if "svp_" in k]) == 7


def test_the_walk_is_shared_not_restated():
    text = open(os.path.join(ROOT, "reak_amd", "csrc", "svp_planner.hip")).read()
    assert "launch_svp_walk(" in text and "svp_walk_points_kernel" not in text
    assert "svp_planner.hip" in open(os.path.join(ROOT, "reak_amd", "csrc", "Makefile")).read().split("OBJ =")[0]
