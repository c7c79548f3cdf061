"""Child process of tests/test_fixup_tiled_gpu.py: batch RRT runs of one scene at forced batch sizes, under whatever
RKH_FIXUP_TILED the parent set; the planner reads its switches when it is created.

    python tests/fixup_worker.py <c1|c1_planar_dyn|c2> <max_vertices> <out.npz> <B> [<B> ...]

c1: the planar arm in its quasi-static space (3 coordinates, rows padded to 4); c1_planar_dyn: the same arm with
dynamics (6 state dimensions); c2: the 6-joint arm with dynamics (12).

Three problems (seeds 1..3) per batch size B; every round takes exactly B candidates (RKH_BATCH_MIN = RKH_BATCH_MAX = B;
B = 1 through a batch factor of 0).  Writes, per B and problem i: b<B>_p<i>_{nn_seq,accept,parent,pos,counts}; counts =
(vertices, iterations, edges checked, solutions, rounds, edges speculated = candidates of all rounds + one goal probe per committed vertex)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from reak_amd import lib, scenarios  # noqa: E402


def main():
    name, max_vertices, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    batches = [int(b) for b in sys.argv[4:]]
    scn = {"c1": lambda: scenarios.make_c1(world_seed=1),
           "c1_planar_dyn": lambda: scenarios.make_c1_planar(world_seed=1, dynamics=True),
           "c2": lambda: scenarios.make_c2(world_seed=1)}[name]()
    ctx = lib.Context(0)
    sc = lib.Scene(ctx, scn)
    qs = lib.make_qs_space(3, scn.meta["lower"], scn.meta["upper"], scn.meta["min_interval"]) if name == "c1" else None
    out = {}
    for B in batches:
        os.environ["RKH_BATCH_MIN"] = str(B)
        os.environ["RKH_BATCH_MAX"] = str(B)
        if B < 8:  # RKH_BATCH_MAX has a floor of 8: a factor of 0 leaves the minimum
            os.environ["RKH_BATCH_FACTOR"] = "0"
        else:
            os.environ.pop("RKH_BATCH_FACTOR", None)
        pl = lib.RrtPlanner(sc, [scn.rrt_params(seed=s, max_vertices=max_vertices) for s in (1, 2, 3)], qs=qs)
        pl.solve_planning_query()
        for i in range(3):
            st, t = pl.all_stats[i], pl.tree(i)
            out[f"b{B}_p{i}_counts"] = np.array([st.num_vertices, st.iterations, st.edges_checked, st.num_solutions, st.rounds,
                                                st.edges_speculated],
                                               dtype=np.int64)
            for key in ("nn_seq", "accept", "parent", "pos"):
                out[f"b{B}_p{i}_{key}"] = t[key]
        pl.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
