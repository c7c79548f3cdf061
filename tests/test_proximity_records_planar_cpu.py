"""Planar proximity records without a GPU: the device's planar closed forms with points compiled for the host against the
oracle's records, the reference side (tests/cpp/prox_record_ref_2d.cpp) against the oracle's own minimum distance, the new
entry points' symbols, the record kernels' resources, and the condition the GPU test's states have to meet."""
import os
import subprocess
import sys

import numpy as np
import pytest

import prox_records_2d as PR2
from reak_amd import scenarios
from reak_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rkh_min_distance_records_2d", "rkh_collision_records_2d")


@pytest.mark.parametrize("routine", sorted(PR2.ROUTINE_KINDS))
def test_planar_closed_forms_on_the_host_match_the_oracles_records(routine):
    """proximity_record_planar_device.h compiled by g++ (tests/cpp/hip_host stands in for the HIP header): 2000 random
    pairs per routine, sizes in make_planar_mixed's ranges, a third each with identity rotations, quarter turns (the
    parallel and perpendicular branches) and random ones, centres close enough that both signs occur.  Points within
    1e-10 max(1, |p|inf) of the oracle's, distances within 1e-12, and the point form's distance is
    pair_distance_planar's bit for bit."""
    a, b = PR2.random_pairs_2d(routine, 2000, 200 + routine)
    ref, got = np.zeros((2000, 5)), np.zeros((2000, 6))
    PR2.ref_lib().prr2_pair_records(a, b, routine, 2000, T.dptr(ref))
    PR2.host_lib().prh2_pair_records(a, b, routine, 2000, T.dptr(got))
    assert np.all(np.isfinite(ref)) and np.all(np.isfinite(got))
    e1, e2 = PR2.point_error(got[:, 0:2], ref[:, 0:2]), PR2.point_error(got[:, 2:4], ref[:, 2:4])
    ed = float(np.max(np.abs(got[:, 4] - ref[:, 4])))
    n_pen = int(np.sum(ref[:, 4] < 0.0))
    print(f"routine {routine}: point1 err {e1:.3e} point2 err {e2:.3e} dist err {ed:.3e} penetrating {n_pen}/2000")
    assert e1 <= PR2.POINT_TOL and e2 <= PR2.POINT_TOL and ed <= PR2.DIST_TOL
    assert np.array_equal(got[:, 4].view(np.uint64), got[:, 5].view(np.uint64))
    if routine == 16:  # rectangle / rectangle is a corner-to-boundary distance without a sign
        assert n_pen == 0
    else:
        assert 100 <= n_pen <= 1900  # both signs are well represented


def test_reference_side_replay_is_the_oracles_minimum_bit_for_bit(oracle):
    """4096 random states of the planar C1 arm: the distance of the min_i that prox_record_ref_2d.cpp's replay of
    proxy_query_model.cpp:163-187 leaves is orc_min_distance's value bit for bit at the oracle's frames.  At the frames
    of the restated chain (tests/kte_ref_planar.py, which the GPU tests use because it knows prismatic joints too) the
    same holds to 1e-12: its frames differ from the oracle's in the last place on a few states."""
    scn = scenarios.make_c1_planar()
    x = PR2.random_states(scn, 4096, 5)
    osc = oracle.OracleScene(scn)
    d = osc.min_distance(x)
    ref = PR2.RefRecords2D(scn)
    rows = np.arange(len(x))
    R = ref.records(PR2.oracle_frames(oracle, scn, x))
    won = R["dist"][rows, R["winner"]]
    assert np.array_equal(won.view(np.uint64), d.view(np.uint64))
    R2 = ref.records(PR2.restated_frames(scn, x))
    assert float(np.max(np.abs(R2["dist"][rows, R2["winner"]] - d))) <= PR2.DIST_TOL
    assert R["dist"].shape[1] == 30 and set(R["routine"]) == {15}
    assert np.any(d < 0.0) and np.any(d > 0.0)


def test_planar_record_entry_points_are_exported_and_declared():
    from reak_amd import lib as L

    L.build()
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "rkh.h")).read()
    for name in ENTRIES:
        assert name in L.EXPORTS and hasattr(lib, name) and name + "(" in header
        assert getattr(lib, name).argtypes is not None
    assert "#define RKH_ABI_VERSION 3u" in header


def test_planar_record_entry_points_refuse_a_null_scene():
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import ctypes as C\n"
        "from reak_amd import lib as L\n"
        "lib = L.load()\n"
        "z = (C.c_double * 12)(); u = (C.c_uint32 * 4)()\n"
        "assert lib.rkh_min_distance_records_2d(None, z, 1, z, z, z, u, u) == -1\n"
        "assert lib.rkh_collision_records_2d(None, z, 1, 1, u, z, z, z, u, u) == -1\n"
        "print('REFUSED')\n" % ROOT)
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "REFUSED" in run.stdout, run.stdout + run.stderr


def test_planar_record_kernels_have_no_spills_and_no_private_segment():
    """One instantiation per chain size serves revolute and prismatic planar chains (SceneDev::prismatic_mask is read at
    run time): none may spill or use a private segment, and no record kernel is a prismatic form."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr

    from reak_amd import lib as L

    L.build()
    res = kr.kernel_resources()
    for n in (1, 2, 3, 4, 6, 7):
        for k in (f"rkh::planar_min_distance_records_kernel<{n}>", f"rkh::planar_collision_records_kernel<{n}>"):
            d = res[k]
            assert d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0 and d["private_segment_fixed_size"] == 0, (k, d)
    assert not [k for k in res if "records_kernel" in k and "prismatic" in k]


@pytest.mark.parametrize("label,make,seed", PR2.gpu_scenes(), ids=[s[0] for s in PR2.gpu_scenes()])
def test_states_of_the_gpu_test_leave_at_most_a_fifth_out_of_the_id_check(label, make, seed):
    """From the reference side alone: of the states the GPU test draws for this scene, the share on which some decision
    of the replay (a gap or a distance against the running minimum) has less than 1e-9 of margin -- those are left out
    of the GPU test's id check -- is at most 0.20, at each of its batch sizes."""
    scn = make()
    ref = PR2.RefRecords2D(scn)
    for B in PR2.GPU_BATCHES:
        x = PR2.random_states(scn, B, seed)
        R = ref.records(PR2.restated_frames(scn, x))
        share = PR2.excluded_share(R)
        won = R["dist"][np.arange(B), R["winner"]]
        undefined = int(np.sum(R["sep"][np.arange(B), R["winner"]] < PR2.MIN_SEPARATION))
        print(f"{label} B={B}: finders={ref.nf} excluded={share:.4f} colliding={int(np.sum(won < 0))} "
              f"winner is not the lowest distance={int(np.sum(won > np.min(R['dist'], axis=1)))} "
              f"winners whose points are undefined={undefined}")
        assert share <= PR2.MAX_EXCLUDED
        assert undefined <= int(PR2.MAX_UNDEFINED * B)  # (prox_records_2d.MIN_SEPARATION: crossing centre lines)
