"""The kernels of svp_space.hip (a module of their own): they exist in the built code objects, spill no vector and no
scalar register and have no private segment -- the nearest sweep keeps the slice's distances in LDS instead of a k-best
list per lane, whose dynamic indexing would need one.  One form of each serves 1 to 12 joints.  The figures are those of
profiles/r21_svp_space_kernel_resources.txt.  Read from the built code objects (tools/kernel_resources.py).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ["rkh::svp_reach_kernel", "rkh::svp_nearest_kernel", "rkh::svp_nearest_merge_kernel", "rkh::svp_walk_solve_kernel",
           "rkh::svp_walk_points_kernel", "rkh::svp_walk_scan_kernel", "rkh::svp_interp_kernel"]
# substrings tests/test_kernel_resources.py picks kernels by, against its own table
RESERVED = ("nn1_", "propagate_pair", "propagate_kernel<6", "edge_points_kernel<6", "edge_check_kernel")


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


def test_svp_kernels_exist_and_spill_nothing(res):
    table = _table("r21_svp_space_kernel_resources.txt")
    built = {k for k in res if "svp_" in k}
    assert built == set(KERNELS) == set(table), built ^ set(KERNELS)
    for k in KERNELS:
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "private segment", d["private_segment_fixed_size"])
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert d["private_segment_fixed_size"] == 0, (k, d)
        assert d["vgpr_count"] <= 128 and d["agpr_count"] == 0, (k, d)   # four waves per SIMD at the least
        assert d["group_segment_fixed_size"] == 0, (k, d)               # the nearest kernels size their LDS at launch
        assert d["max_flat_workgroup_size"] == 256, (k, d)
        assert table[k][:6] == [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"],
                                d["private_segment_fixed_size"], d["group_segment_fixed_size"]], (k, table[k], d)


def test_svp_kernel_names_keep_clear_of_the_committed_table():
    for k in KERNELS:
        assert not [s for s in RESERVED if s in k], k


def test_nearest_lds_fits_a_block():
    """the largest slice: 4096 distances, the query (24 doubles), the reduction (4 doubles + 8 words): under the 64 KB a
    launch gets without asking; the merge: 4096 cursors"""
    text = open(os.path.join(ROOT, "reak_amd", "csrc", "svp_space.hip")).read()
    assert "constexpr uint32_t kSvpSliceMax = 4096;" in text and "constexpr uint32_t kSvpMaxSlices = 4096;" in text
    assert (4096 + 24 + 4) * 8 + 8 * 4 <= 64 * 1024 and 4 * 8 + (8 + 4096) * 4 <= 64 * 1024
