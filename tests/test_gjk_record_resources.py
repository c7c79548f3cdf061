"""The record kernels after the mesh forms were added (propagate.hip: min_distance_records_meshes_kernel,
collision_records_meshes_kernel, instantiated from the bodies the closed-form kernels share with them): the closed-form
kernels must be the code they were -- registers, scratch and LDS of profiles/r16_record_kernel_resources.txt, taken from
the build of the parent commit -- and the mesh forms may spill nothing: their private segment is that of the support-map
search's run-time-indexed simplex arrays, as in the mesh edge-walk kernel.  Read from the built code objects
(tools/kernel_resources.py).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CHAINS = (1, 2, 3, 4, 6, 7, 12)


@pytest.fixture(scope="module")
def res():
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    return kr.kernel_resources()


@pytest.fixture(scope="module")
def table():
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "r16_record_kernel_resources.txt")):
        if line.startswith("#") or line.startswith("kernel") or not line.strip():
            continue
        rows[line[:78].strip()] = [int(x) for x in line[78:].split()]
    return rows


def _figures(d):
    return [d["vgpr_count"], d["agpr_count"], d["vgpr_spill_count"], d["sgpr_count"], d["private_segment_fixed_size"],
            d["group_segment_fixed_size"]]


@pytest.mark.parametrize("kernel", ["min_distance_records_kernel", "collision_records_kernel"])
def test_closed_form_record_kernels_did_not_move(res, table, kernel):
    for n in CHAINS:
        k = f"rkh::{kernel}<{n}>"
        assert table[k][:6] == _figures(res[k]), (k, table[k], res[k])
        assert res[k]["private_segment_fixed_size"] == 0 and res[k]["vgpr_spill_count"] == 0


@pytest.mark.parametrize("kernel", ["min_distance_records_meshes_kernel", "collision_records_meshes_kernel"])
def test_mesh_record_kernels_spill_nothing_beyond_the_simplex_arrays(res, table, kernel):
    """No spilled vector or scalar register; the private segment holds the simplex of the search (4 points), the simplex
    and the support points of the record with their copies (16 points) and the face loop's candidates: well under 1 KB.
    One wave per state with one block per state: the registers (<= 256) allow two waves per SIMD."""
    for n in CHAINS:
        k = f"rkh::{kernel}<{n}>"
        d = res[k]
        print(k, "vgpr", d["vgpr_count"], "sgpr", d["sgpr_count"], "private segment", d["private_segment_fixed_size"], "B")
        assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (k, d)
        assert 0 < d["private_segment_fixed_size"] <= 1024, (k, d)
        assert d["vgpr_count"] <= 256 and d["agpr_count"] == 0, (k, d)
        assert table[k][:6] == _figures(d), (k, table[k], d)


def test_the_committed_table_lists_the_record_kernels_of_the_build(res, table):
    built = {k for k in res if "records" in k and "planar" not in k and "gjk_pair" not in k}
    assert built == set(table), built ^ set(table)
    assert len(table) == 4 * len(CHAINS)
