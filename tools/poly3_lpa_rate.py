"""Numbers of the 3-D moving-obstacle LPA* (no gate): the replanner flow on replanner_world3 -- set_worlds, update_nodes, plan,
sub_state_space(1), 8 ticks -- for ACC, ACC + turn and JRK + turn with the 27-input lattice.  Per tick: the LPA* plan's expansions
and kernel milliseconds (PolyLpa3D.last_kernel_ms) next to those of a fresh PolyTeam3D.plan_batch on the same world; medians over
the repetitions of the whole flow.  Prints one JSON line per case.
usage: python tools/poly3_lpa_rate.py [--reps N]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd import poly_map3d as p3  # noqa: E402

KW = {p3.ACC: dict(dt=1.0, v_max=2.0, a_max=1.0, w=10.0), p3.JRK: dict(dt=1.0, v_max=2.0, a_max=1.0, j_max=1.0, w=10.0)}
CASES = [("ACC", p3.ACC, False), ("ACC+turn", p3.ACC, True), ("JRK+turn", p3.JRK, True)]


def flow(control, turn):
    """one pass of the replanner flow -> per tick (LPA* expansions, LPA* ms, fresh expansions, fresh ms, entries changed)"""
    team = p3.PolyTeam3D()
    team.configure(control, p3.U27, **KW[control])
    team.set_worlds([p3.replanner_world3(0.0, turn)])
    team.set_capacity(1, 1 << 16, 1 << 19, 1 << 19)
    l = team.lpa()
    l.set_capacity(1 << 16, 1 << 20, 1 << 20)
    start, goal = p3.replanner_endpoints3()
    t, rows = 0.0, []
    for tick in range(8):
        team.set_worlds([p3.replanner_world3(t, turn)])
        nb, nc, _ = l.update_nodes()
        ok = l.plan(start, goal)
        lpa = (int(l.result.n_expanded), l.last_kernel_ms())
        ra = team.plan_batch([0], [start], [goal], max_expand=-1)[0]
        assert ra.status == l.result.status and ra.cost == l.result.cost, (tick, ra.status, l.result.status, ra.cost, l.result.cost)
        rows.append(lpa + (int(ra.n_expanded), team.last_kernel_ms(), nb + nc))
        act, ids, st = l.traj()
        if not ok or len(act) <= 2:
            break
        l.sub_state_space(1)
        start = st[1].copy()
        t += 1.0
        start[12] = t
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    flow(p3.ACC, False)  # warm-up
    for name, control, turn in CASES:
        runs = [flow(control, turn) for _ in range(a.reps)]
        ticks = []
        for k in range(len(runs[0])):
            ticks.append({"tick": k, "lpa_expansions": runs[0][k][0], "lpa_kernel_ms": round(float(np.median([r[k][1] for r in runs])), 3),
                          "fresh_expansions": runs[0][k][2], "fresh_kernel_ms": round(float(np.median([r[k][3] for r in runs])), 3),
                          "entries_changed": runs[0][k][4]})
        first = ticks[0]["lpa_kernel_ms"] / ticks[0]["fresh_kernel_ms"]
        print(json.dumps({"case": name, "reps": a.reps, "first_plan_over_fresh": round(first, 2),
                          "repairs_lpa_ms": round(sum(x["lpa_kernel_ms"] for x in ticks[1:]), 3),
                          "repairs_fresh_ms": round(sum(x["fresh_kernel_ms"] for x in ticks[1:]), 3), "ticks": ticks}))


if __name__ == "__main__":
    main()
