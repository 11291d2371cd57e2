"""Numbers of the moving-obstacle LPA* fleet (no gate): a tick of N robots that each keep an LPA* space -- updateNodes + plan -- as one
PolyLpaFleet call pair against the same calls on N single PolyLpa handles one after the other (that path's code is what it was before
the fleet existed).  The members and the flow are those of tests/test_plpa_fleet.py: the 16 ACC members of
tests/golden/plpa_fleet_pairs.json on pm.replanner_world, eight ticks (reload the world at t, updateNodes, plan, getSubStateSpace(1), on
from the second state); N = 64 repeats the list four times.  Per N the whole flow is run --reps times on both sides in one process,
the order of the sides alternating per tick and repetition; the world commits and getSubStateSpace are outside the timed region.  Per
tick of repairs (ticks 2..8): wall ms of updateNodes + plan with its spread, kernel ms (fleet: the search launch and the updateNodes
launch; singles: the sum of the members' search launches -- the single handle does not time its updateNodes launch), the longest
member's expansions.  --cpu: the CPU checker's one-thread time for the same repairs (a restatement on ONE core, not the device's
competitor; its 16 distinct members are timed once and N = 64 is four times that).
usage: python tools/plpa_fleet_rate.py [--reps 10] [--sizes 1,16,64] [--cpu]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpl_ros_amd import poly_map as pm  # noqa: E402
from tests import test_plpa_fleet as T  # noqa: E402


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def timed_tick(side, starts, goals):
    """updateNodes + plan on one side -> (wall ms, kernel ms of the searches, kernel ms of the updateNodes launch or None, results)"""
    t0 = time.perf_counter()
    side.update()
    res = side.plan(starts, goals)
    wall = (time.perf_counter() - t0) * 1e3
    if side.fleet:
        k_plan, k_upd = side.fleet.last_kernel_ms()
        return wall, k_plan, k_upd, res
    return wall, sum(l.last_kernel_ms() for l in side.singles), None, res


def cpu_ticks(members):
    """one-thread ms of updateNodes + plan per tick, summed over the members, on the CPU checker"""
    from oracle import refpoly
    ms = np.zeros(T.TICKS)
    for turn, start, goal in members:
        R = refpoly.RefWorld(pm.replanner_world(0.0, turn), pm.ACC, pm.U9, **T.KW[pm.ACC])
        R.lpa_reset()
        start, t = start.copy(), 0.0
        for tick in range(T.TICKS):
            R.reload(pm.replanner_world(t, turn))
            t0 = time.perf_counter()
            R.lpa_update_nodes()
            ro = R.lpa_plan(start, goal, max_expand=T.MAX_EXPAND)
            ms[tick] += (time.perf_counter() - t0) * 1e3
            ss = R.lpa_state_space()
            R.lpa_sub_state_space(1)
            start = ss["states"][ro["node_ids"][1]].copy()
            t += 1.0
            start[8] = t
        R.lpa_reset()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--cpu", action="store_true", help="also time the CPU checker's LPA* (one thread) on the same repairs")
    a = ap.parse_args()
    base = T.acc_members()
    report = {"reps": a.reps, "sizes": {}}
    cpu16 = cpu_ticks(base) if a.cpu else None
    cpu1 = cpu_ticks(base[:1]) if a.cpu else None
    for N in [int(x) for x in a.sizes.split(",")]:
        members = [base[i % len(base)] for i in range(N)]
        world_of = [int(m[0]) for m in members]
        sides = {"fleet": T.Side(pm.ACC, world_of, fleet=True), "singles": T.Side(pm.ACC, world_of, fleet=False)}
        rows = {k: [[] for _ in range(T.TICKS)] for k in sides}
        longest = [0] * T.TICKS
        for rep in range(a.reps + 1):  # (the first repetition warms up and is not counted)
            starts = [m[1].copy() for m in members]
            goals = [m[2] for m in members]
            t = 0.0
            for tick in range(T.TICKS):
                for s in sides.values():
                    s.set_worlds(t)
                order = ("fleet", "singles") if (rep + tick) % 2 == 0 else ("singles", "fleet")
                got = {k: timed_tick(sides[k], starts, goals) for k in order}
                assert got["fleet"][3] == got["singles"][3], (N, rep, tick)  # the same searches on both sides
                assert sides["fleet"].fleet.stats()[1] == 1
                longest[tick] = max(int(r["n_expanded"]) for r in got["fleet"][3])
                if rep > 0:
                    for k in sides:
                        rows[k][tick].append(got[k][:3])
                trajs = [sides["fleet"].member(i).traj() for i in range(N)]
                for s in sides.values():
                    s.sub([1] * N)
                t += 1.0
                for i in range(N):
                    starts[i] = trajs[i][2][1].copy()
                    starts[i][8] = t
        out = {"ticks": []}
        print(f"N={N:3d}  (tick 1 plans afresh; ticks 2..8 repair) wall / kernel ms of updateNodes + plan, median [min .. max] of {a.reps} repetitions", flush=True)
        for tick in range(T.TICKS):
            row = {"tick": tick + 1, "longest_member_expansions": longest[tick]}
            line = f"  tick {tick + 1}: longest member {longest[tick]:5d} expansions"
            for k in ("fleet", "singles"):
                wall, kp, ku = zip(*rows[k][tick])
                row[k] = {"wall_ms": spread(wall), "plan_kernel_ms": spread(kp)}
                line += (f"\n      {k:8s} wall {row[k]['wall_ms']['median']:9.3f} [{row[k]['wall_ms']['min']:.3f} .. {row[k]['wall_ms']['max']:.3f}]"
                         f"  search kernel {row[k]['plan_kernel_ms']['median']:9.3f} [{row[k]['plan_kernel_ms']['min']:.3f} .. {row[k]['plan_kernel_ms']['max']:.3f}]")
                if k == "fleet":
                    row[k]["update_kernel_ms"] = spread(ku)
                    line += f"  updateNodes kernel {row[k]['update_kernel_ms']['median']:.3f} [{row[k]['update_kernel_ms']['min']:.3f} .. {row[k]['update_kernel_ms']['max']:.3f}]"
            row["wall_ratio_singles_over_fleet"] = row["singles"]["wall_ms"]["median"] / row["fleet"]["wall_ms"]["median"]
            line += f"\n      singles / fleet wall: {row['wall_ratio_singles_over_fleet']:.2f}"
            if a.cpu:
                row["cpu_checker_one_thread_ms"] = float(cpu1[tick] if N == 1 else cpu16[tick] * N / len(base))
                line += f"   CPU checker, one thread (a restatement, one core): {row['cpu_checker_one_thread_ms']:.3f} ms"
            out["ticks"].append(row)
            print(line, flush=True)
        rep_f = [np.median([x[0] for x in rows["fleet"][k]]) for k in range(1, T.TICKS)]
        rep_s = [np.median([x[0] for x in rows["singles"][k]]) for k in range(1, T.TICKS)]
        out["repair_ticks_mean_wall_ms"] = {"fleet": float(np.mean(rep_f)), "singles": float(np.mean(rep_s))}
        print(f"  mean over the repair ticks 2..8: fleet {np.mean(rep_f):.3f} ms, singles {np.mean(rep_s):.3f} ms per tick of {N}"
              + (f", CPU checker {float(np.mean((cpu1 if N == 1 else cpu16 * N / len(base))[1:])):.3f} ms" if a.cpu else ""), flush=True)
        report["sizes"][str(N)] = out
        del sides
        gc.collect()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
