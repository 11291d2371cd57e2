"""Numbers of the state-space export of the 2-D moving-obstacle A* (no gate): kernel time of the three export passes
(mplx_poly_result_nodes / _edges / _blocked: HIP-event times of the first pass with its scan, the edges pass, the blocked pass)
next to the plan's own kernel time, and the bytes that cross the bus, on
  * the capped open-world query of tests/test_poly_space.py (38 k states, 108 k predecessor records: two chunks of each), and
  * the 16-robot tick of BASELINE config 5 (poly_map.team2_tick), every robot's space exported.
`whole_records_bytes` is what copying the query's node and predecessor records whole would move (the host getters' route).
Medians over --reps fresh plans (a new plan drops the cached export).  usage: python tools/poly_space_rate.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd import poly_map as pm  # noqa: E402
from tests import test_poly_space as tps  # noqa: E402


def export_all(team, R):
    """export every query's space; returns (kernel ms [first pass, edges, blocked], wall s, bytes down, whole-record bytes)"""
    ms, down, whole = np.zeros(3), 0, 0
    t0 = time.perf_counter()
    for q, r in enumerate(R):
        if r.n_nodes == 0:
            continue
        sp = team.state_space(q)
        a = np.array(team.space_kernel_ms())
        bp, _ = team.blocked(q)
        ms += np.array([a[0], a[1], team.space_kernel_ms()[2]])
        n, m = sp["n_nodes"], len(sp["child"])
        down += n * (9 * 8 + 8 + 8 + 1) + m * 12 + n * 4
        whole += n * 128 + m * 12
    return ms, time.perf_counter() - t0, down, whole


def measure(team, world_of, starts, goals, reps, **kw):
    team.plan_batch(world_of, starts, goals, **kw)  # warm-up
    export_all(team, team._results)
    plan_ms, exp_ms, wall, down, whole = [], [], [], 0, 0
    for _ in range(reps):
        R = team.plan_batch(world_of, starts, goals, **kw)
        plan_ms.append(team.last_kernel_ms())
        ms, w, down, whole = export_all(team, R)
        exp_ms.append(ms)
        wall.append(w)
    e = np.median(np.array(exp_ms), axis=0)
    return {"plan_kernel_ms": float(np.median(plan_ms)), "first_pass_ms": float(e[0]), "edges_pass_ms": float(e[1]), "blocked_pass_ms": float(e[2]),
            "export_wall_ms": float(np.median(wall)) * 1e3, "bytes_down": int(down), "whole_records_bytes": int(whole),
            "n_nodes": int(sum(r.n_nodes for r in R)), "n_edges": int(sum(r.n_edges for r in R)), "queries": len(R)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = {}
    s, g = tps.open_query()
    team = tps.make_team(pm.ACC, pm.U9, tps.OPEN_ENV, [tps.open_world()])
    out["open_world_capped"] = measure(team, [0], [s], [g], a.reps, eps=0.0, max_expand=tps.CHUNK_CAP)
    worlds, starts, goals = pm.team2_tick()
    team = pm.PolyTeam()
    team.configure(pm.ACC, pm.U9, dt=0.5, v_max=2.0, a_max=1.0, w=10.0)  # (the set-up of benchmarks/c5.py: the reference's parameters)
    team.set_worlds(worlds)
    team.set_capacity(16, 1 << 21, 1 << 23, 1 << 22)
    team.set_deadline(120.0)
    out["c5_tick_16_robots"] = measure(team, list(range(16)), starts, goals, a.reps, eps=1.0, tol_pos=0.5, max_expand=-1, heur_ignore_dynamics=False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
