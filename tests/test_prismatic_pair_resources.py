"""The prismatic forms of the two-lanes-per-edge steer kernels (propagate_pair_prismatic.hip, namespace rkh::prismatic,
built into reak_amd/librkh_prismatic_pair.so) must keep what the mapping is designed around, like the revolute forms
(tests/test_kernel_resources.py): two waves per SIMD (<= 256 registers per lane), eight waves per CU (LDS), no spilled
registers and no private segment.  Read from the built code objects (tools/kernel_resources.py).  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def res():
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    res = kr.kernel_resources()  # the revolute forms, for the LDS comparison
    res.update(kr.kernel_resources(kr.PRISMATIC_PAIR_SO))
    return res


@pytest.mark.parametrize("n", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("kernel", ["propagate_pair_kernel", "propagate_pair_step_kernel"])
def test_prismatic_pair_kernels_hold_two_waves_per_simd_without_scratch(res, kernel, n):
    import kernel_resources as kr

    k = f"rkh::prismatic::{kernel}<{n}>"
    assert k in res, k
    d = res[k]
    assert d["vgpr_count"] <= 256 and d["agpr_count"] == 0, (k, d)
    assert d["vgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (k, d)
    assert kr.waves_per_simd(d) == 2, (k, d)
    assert d["group_segment_fixed_size"] * 8 <= 160 * 1024, (k, d)


def test_prismatic_pair_forms_add_no_lds(res):
    """The prismatic root's end position is recomputed, not stored: the forms use the LDS of the revolute ones."""
    for n in (1, 2, 3, 4, 6, 7):
        for kernel in ("propagate_pair_kernel", "propagate_pair_step_kernel"):
            assert res[f"rkh::prismatic::{kernel}<{n}>"]["group_segment_fixed_size"] == res[f"rkh::{kernel}<{n}>"]["group_segment_fixed_size"]
    for n in (3, 6, 7):
        assert res[f"rkh::prismatic::pair_counts_kernel<{n}>"]["group_segment_fixed_size"] == \
            res[f"rkh::pair_counts_kernel<{n}>"]["group_segment_fixed_size"]


def test_prismatic_pair_library_holds_the_pair_forms_only():
    """librkh_prismatic_pair.so carries the kernels of propagate_pair_prismatic.hip and nothing else, and librkh.so
    none of them."""
    import kernel_resources as kr

    own = kr.kernel_resources(kr.PRISMATIC_PAIR_SO)
    assert len(own) == 15, sorted(own)  # 6 + 6 steer kernels, the count probe for 3, 6 and 7 joints
    for k in own:
        assert k.split("<")[0] in ("rkh::prismatic::propagate_pair_kernel", "rkh::prismatic::propagate_pair_step_kernel",
                                   "rkh::prismatic::pair_counts_kernel"), k
    assert not [k for k in kr.kernel_resources() if k in own]
