"""Generates tests/golden/steer_filters_track.npz: the steered edges of the CRS A465 track robot at the origin and 1e5 m
away from it, by the test-side restatement (tests/kte_ref.py; 70 ms per edge in Python, about a minute in all).
tests/test_steer_filters_cpu.py recomputes a few of the edges and compares them.  With `states` as its argument it
generates tests/golden/steer_filters_track_states.npz instead: states of that robot on either side of contact.
Run:  python tests/make_steer_filter_golden.py [states]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import oracle_lib  # noqa: E402
import steer_filter_scenes  # noqa: E402

if __name__ == "__main__":
    oracle_lib.build()
    if sys.argv[1:] == ["states"]:
        steer_filter_scenes.make_track_contacts(oracle_lib)
    else:
        steer_filter_scenes.write_track_golden(oracle_lib)
