"""The depth forms of the record kernels (propagate_depth.hip: min_distance_depth_kernel, collision_depth_kernel and the
pair-by-pair gjk_pair_depth_kernel, over the record bodies of propagate_records.h in a module of their own): they spill no vector
and no scalar register, stay within 256 registers, and their private segment is what the polytope cap of
reak_amd/csrc/epa_device.h implies.  The figures are those of profiles/r17_depth_kernel_resources.txt.  The kernels that
existed before must be the code they were: every row of profiles/r03_kernel_resources.txt and
profiles/r16_record_kernel_resources.txt still holds.  Read from the built code objects (tools/kernel_resources.py).  No GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CHAINS = (1, 2, 3, 4, 6, 7, 12)
SIMPLEX_BYTES = 1024   # the bound tests/test_gjk_record_resources.py holds the search's simplex arrays to


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


def _figures(d):
    return [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"], d["private_segment_fixed_size"],
            d["group_segment_fixed_size"]]


def _cap():
    """kEpaMaxVerts, and the bytes of polytope arrays per vertex the header states."""
    text = open(os.path.join(ROOT, "reak_amd", "csrc", "epa_device.h")).read()
    cap = int(re.search(r"constexpr int kEpaMaxVerts = (\d+);", text).group(1))
    # EpaVert: two d3 (48 bytes); EpaFace: d3, double, three indices, padded to 40, two per vertex; horizon: 2 bytes
    return cap, 48 + 2 * 40 + 2


def test_depth_kernels_spill_nothing_and_fit_the_cap(res):
    table = _table("r17_depth_kernel_resources.txt")
    cap, per_vertex = _cap()
    names = [f"rkh::{k}<{n}>" for k in ("min_distance_depth_kernel", "collision_depth_kernel") for n in CHAINS]
    names.append("rkh::gjk_pair_depth_kernel")
    for k in names:
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "private segment", d["private_segment_fixed_size"], "B of",
              cap * per_vertex, "+", SIMPLEX_BYTES)
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert d["vgpr_count"] <= 256 and d["agpr_count"] == 0, (k, d)
        assert cap * per_vertex <= d["private_segment_fixed_size"] <= cap * per_vertex + SIMPLEX_BYTES, (k, d)
        assert table[k][:6] == _figures(d), (k, table[k], d)
    built = {k for k in res if "depth" in k}
    assert built == set(table) == set(names), built ^ set(table)


def test_the_depth_kernels_are_not_record_kernels_by_name(res):
    """tests/test_gjk_record_resources.py counts the kernels with `records` in their name against its own table."""
    assert not [k for k in res if "depth" in k and "records" in k]


@pytest.mark.parametrize("name", ["r03_kernel_resources.txt", "r16_record_kernel_resources.txt"])
def test_no_kernel_that_existed_moved(res, name):
    import kernel_resources as kr

    table = _table(name)
    built = dict(res)
    built.update(kr.kernel_resources(kr.PRISMATIC_PAIR_SO))   # the tables cover both libraries
    built = {k[:78]: v for k, v in built.items()}             # and cut the names at 78 characters
    moved = {k: (v[:6], _figures(built[k]) if k in built else None) for k, v in table.items()
             if k not in built or v[:6] != _figures(built[k])}
    assert len(table) >= 28 and not moved, moved
