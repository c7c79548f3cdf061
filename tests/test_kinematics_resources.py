"""The kinematics kernels (kinematics_frames.hip, a module of their own): they exist in the built code objects, and they spill
no vector and no scalar register and have no private segment.  One form of each serves every chain length -- nothing is
kept per joint in registers or private memory -- so these figures ARE the figures for chains of at most 7 joints, and of
12.  The figures are those of profiles/r20_kinematics_kernel_resources.txt.  That no kernel that existed before moved is
tests/test_depth_record_resources.py::test_no_kernel_that_existed_moved's to say.  Read from the built code objects
(tools/kernel_resources.py).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KERNELS = ["rkh::kinematics_frames_kernel<false>", "rkh::kinematics_frames_kernel<true>",
           "rkh::kinematics_frames_planar_kernel<false>", "rkh::kinematics_frames_planar_kernel<true>",
           "rkh::kinematics_ik_kernel"]
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


def test_kinematics_kernels_exist_and_spill_nothing(res):
    table = _table("r20_kinematics_kernel_resources.txt")
    built = {k for k in res if "kinematics" in k}
    assert built == set(KERNELS) == set(table), built ^ set(KERNELS)
    for k in KERNELS:
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "private segment", d["private_segment_fixed_size"])
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert d["private_segment_fixed_size"] == 0, (k, d)
        assert d["vgpr_count"] <= 256 and d["agpr_count"] == 0, (k, d)   # two waves per SIMD at the least
        assert d["group_segment_fixed_size"] == 0, (k, d)               # the IK kernel's LDS is dynamic: 8 n doubles per lane
        assert d["max_flat_workgroup_size"] == 64, (k, d)
        assert table[k][:6] == [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"],
                                d["private_segment_fixed_size"], d["group_segment_fixed_size"]], (k, table[k], d)


def test_kinematics_kernel_names_keep_clear_of_the_committed_table(res):
    for k in KERNELS:
        assert not [s for s in RESERVED if s in k], k


def test_ik_lds_fits_a_block_for_every_chain():
    """8 n doubles per lane, 64 lanes: 48 KB for the longest chain a scene holds, under the 64 KB a launch gets without asking."""
    text = open(os.path.join(ROOT, "reak_amd", "csrc", "kinematics_device.h")).read()
    assert "constexpr int kKinMaxDof = 12;" in text
    assert 8 * 12 * 64 * 8 <= 64 * 1024
