#!/usr/bin/env python3
"""Writes tests/golden/plpa_fleet_pairs.json: the members of the moving-obstacle LPA* fleet tests (tests/test_plpa_fleet.py).  Settings
only: the eight (start -> goal) pairs on pm.replanner_world, the two pairs whose first plan runs into the cap, and the JRK members --
the first four candidates (pair x turn, in list order) that complete the eight-tick flow on the CPU checker (oracle/refpoly.py) with
status 0 on every tick and at least one repair that expands a state.  usage: tools/make_plpa_fleet_pairs.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpl_ros_amd import poly_map as pm  # noqa: E402
from tests import test_plpa_fleet as T  # noqa: E402

PAIRS = [[[0.5, 2], [19, 8]], [[19.5, 2], [1, 12]], [[0.5, 4], [19, 10]], [[19.5, 8], [1, 2]],
         [[0.5, 10], [19, 16]], [[19.5, 10], [1, 4]], [[0.5, 14], [19, 4]], [[19.5, 14], [1, 8]]]
CAPPED = [[[19.5, 4], [1, 14]], [[0.5, 8], [19, 14]]]

if __name__ == "__main__":
    jrk, tried = [], []
    for s, g in PAIRS:
        for turn in (False, True):
            if len(jrk) == 4:
                break
            recs = T.checker_flow(pm.JRK, (turn, T.state9(s), T.state9(g)), keep_spaces=False)
            complete, first, rep, changed, nmax = T.flow_facts(recs)
            ok = complete and rep > 0 and changed > 0 and nmax <= T.CAP[0]
            tried.append(dict(turn=turn, start=s, goal=g, ticks=len(recs), statuses=[r["plan"]["status"] for r in recs], first=first, repairs=rep, largest=nmax, kept=ok))
            print(tried[-1])
            if ok:
                jrk.append([turn, s, g])
    out = dict(world="pm.replanner_world(t, turn), scale 1", lattice="pm.U9", max_expand=T.MAX_EXPAND, ticks=T.TICKS,
               pairs=PAIRS, capped_pairs=CAPPED, jrk_members=jrk, jrk_candidates_tried=tried)
    with open(T.FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{T.FIXTURE}: {len(PAIRS)} pairs, {len(CAPPED)} capped pairs, {len(jrk)} JRK members of {len(tried)} candidates tried")
