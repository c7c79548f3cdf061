"""Proximity records without a GPU: the reference side (tests/cpp/prox_record_ref.cpp) against the oracle's own minimum
distance, the device's closed forms with points compiled for the host against the oracle's, the new entry points'
symbols and their loud failure without a GPU, and the record kernels' resources."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import prox_records as PR
from reak_amd import scenarios
from reak_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_side_winner_is_the_oracles_minimum_bit_for_bit(oracle):
    """4096 random C2 states: the distance of the winner of the loop of proxy_query_model.cpp:376-400, as
    prox_record_ref.cpp replays it over the oracle's records, is orc_min_distance's value bit for bit; the winner is the
    first finder at that distance."""
    scn = scenarios.make_c2()
    x = PR.random_states(scn, 4096, 5)
    osc = oracle.OracleScene(scn)
    R = PR.RefRecords(scn).records(osc.fk(x))
    d = osc.min_distance(x)
    rows = np.arange(len(x))
    won = R["dist"][rows, R["winner"]]
    assert np.array_equal(won.view(np.uint64), d.view(np.uint64))
    assert np.array_equal(R["winner"], np.argmin(R["dist"], axis=1))  # argmin: the first of equal minima
    assert R["dist"].shape[1] == 300 and set(R["routine"]) == {2, 4, 5}


@pytest.mark.parametrize("routine", sorted(PR.ROUTINE_KINDS))
def test_device_closed_forms_on_the_host_match_the_oracles_records(routine):
    """proximity_record_device.h compiled by g++ (tests/cpp/hip_host stands in for the HIP header): 2000 random pairs per
    routine, sizes in make_c2's ranges, a third each with identity orientations, quarter turns (parallel and
    perpendicular axes) and random ones, centres close enough that many penetrate.  Points within 1e-10 max(1, |p|inf) of
    the oracle's, distances within 1e-12 -- both compute in the same operation order, so they are in fact equal -- and the
    point form's distance is pair_distance's bit for bit."""
    a, b = PR.random_pairs(routine, 2000, 100 + routine)
    ref, got = np.zeros((2000, 7)), np.zeros((2000, 8))
    PR.ref_lib().prr_pair_records(a, b, routine, 2000, T.dptr(ref))
    PR.host_lib().prh_pair_records(a, b, routine, 2000, T.dptr(got))
    first = C.c_int(0)
    assert PR.host_lib().prh_pair_routine(a[0].kind, b[0].kind, C.byref(first)) == routine and first.value == 1
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    e1, e2 = PR.point_error(got[:, 0:3], ref[:, 0:3]), PR.point_error(got[:, 3:6], ref[:, 3:6])
    ed = float(np.max(np.abs(got[:, 6] - ref[:, 6])))
    n_pen = int(np.sum(ref[:, 6] < 0.0))
    print(f"routine {routine}: point1 err {e1:.3e} point2 err {e2:.3e} dist err {ed:.3e} penetrating {n_pen}/2000")
    assert e1 <= PR.POINT_TOL and e2 <= PR.POINT_TOL and ed <= PR.DIST_TOL
    assert np.array_equal(got[:, 6].view(np.uint64), got[:, 7].view(np.uint64))
    if routine != 6:  # (prox_plane_plane's distance has no sign: the nearest corner's, never below 0)
        assert 100 <= n_pen <= 1900  # both signs are well represented


def test_record_entry_points_are_exported_and_declared():
    from reak_amd import lib as L

    L.build()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "rkh.h")).read()
    for name in ("rkh_min_distance_records", "rkh_collision_records"):
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header
        assert getattr(lib, name).argtypes is not None
    assert "#define RKH_ABI_VERSION 3u" in header


def test_record_entry_points_fail_loudly_without_a_gpu():
    """Like every call of the binding: on a machine without a GPU the context cannot be created and the scene methods are
    never reached with a handle; called with no scene at all the entries refuse the NULL instead of touching it."""
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import ctypes as C\n"
        "import numpy as np\n"
        "from reak_amd import lib as L\n"
        "lib = L.load()\n"
        "z = (C.c_double * 12)(); u = (C.c_uint32 * 4)()\n"
        "assert lib.rkh_min_distance_records(None, z, 1, z, z, z, u, u) == -1\n"
        "assert lib.rkh_collision_records(None, z, 1, 1, u, z, z, z, u, u) == -1\n"
        "try:\n"
        "    L.Context(0)\n"
        "except Exception as e:\n"
        "    print('LOUD', type(e).__name__)\n"
        "else:\n"
        "    print('HAS_GPU')\n" % ROOT)
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "LOUD" in run.stdout or "HAS_GPU" in run.stdout


def test_record_kernels_have_no_spills_and_no_private_segment():
    """One instantiation per chain size in the revolute translation unit serves prismatic chains too (none is added to
    rkh::prismatic); none may spill or use a private segment."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    from reak_amd import lib as L

    L.build()
    res = kr.kernel_resources()
    for n in (1, 2, 3, 4, 6, 7, 12):
        for k in (f"rkh::min_distance_records_kernel<{n}>", f"rkh::collision_records_kernel<{n}>"):
            d = res[k]
            assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (k, d)
    assert not [k for k in res if "records_kernel" in k and "prismatic" in k]
