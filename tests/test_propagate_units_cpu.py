"""The four translation units over propagate.hip's former text (propagate.hip, propagate_prismatic.hip,
propagate_planar_qs_prismatic.hip, propagate_depth.hip) are ordinary source files over shared headers, and splitting them
moved no kernel: every kernel of the two libraries has the resources it had in the parent commit's build
(profiles/r23_kernel_resources_parent.txt, written by tools/kernel_resources.py --out from that build and committed
unchanged), and the libraries hold the same set of kernels.  The instruction-level comparison is
tools/compare_kernel_code.py (profiles/r23_propagate_units_code_identity.txt).  No GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reak_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def rows():
    """The resource table of this build, in the committed table's own format: {kernel name as printed: row}."""
    import kernel_resources as kr

    from reak_amd import lib

    lib.build()
    res = kr.kernel_resources()
    res.update(kr.kernel_resources(kr.PRISMATIC_PAIR_SO))
    return _rows(kr.table(res).splitlines())


def _rows(lines):
    out = {}
    for line in lines:
        if line.startswith("#") or line.startswith("kernel") or not line.strip():
            continue
        assert line[:78] not in out, line
        out[line[:78]] = line
    return out


@pytest.fixture(scope="module")
def parent_rows():
    return _rows(open(os.path.join(ROOT, "profiles", "r23_kernel_resources_parent.txt")).read().splitlines())


def test_every_kernel_keeps_its_resource_row(rows, parent_rows):
    moved = [(parent_rows[k], rows[k]) for k in sorted(set(rows) & set(parent_rows)) if rows[k] != parent_rows[k]]
    assert not moved, moved


def test_the_set_of_kernels_is_unchanged(rows, parent_rows):
    assert len(parent_rows) > 400
    assert sorted(rows) == sorted(parent_rows), (sorted(set(parent_rows) - set(rows)), sorted(set(rows) - set(parent_rows)))


def test_units_are_plain_files():
    """Only the two-lanes and the planar steer kernels are still a text compiled a second time by a wrapper unit; no unit
    includes another one otherwise, and the macros that selected a regime of propagate.hip are gone."""
    including = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h", ".inl")) and name != "Makefile":
            continue
        text = open(os.path.join(CSRC, name), errors="replace").read()
        for macro in ("RKH_PLANAR_PRISMATIC_QS", "RKH_DEPTH_RECORDS", "RKH_FORMS_ONLY"):
            assert macro not in text, (name, macro)
        if name.endswith(".hip") and re.search(r'^\s*#\s*include\s*"[^"]*\.hip"', text, re.M):
            including.append(name)
    assert including == ["propagate_pair_prismatic.hip", "propagate_planar_prismatic.hip"]
