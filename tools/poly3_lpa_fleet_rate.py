"""Numbers of the 3-D moving-obstacle LPA* fleet (no gate): a tick of N robots that each keep an LPA* space -- updateNodes + plan -- as
one PolyLpaFleet3D call pair against the same calls on N single PolyLpa3D handles one after the other, on the same build.  The members
and the flow are those of tests/test_poly3_lpa_fleet.py: its 8 ACC members on p3.replanner_world3, five ticks (commit the worlds at t,
updateNodes, plan, getSubStateSpace(1), on from the second state); a larger N repeats the list.  Per N the whole flow is run --reps
times on both sides in one process (after one repetition that warms up), the order of the sides alternating per tick and repetition;
the world commits and getSubStateSpace are outside the timed region.  Per tick: wall ms of updateNodes + plan, kernel ms (fleet: the
search launch and the updateNodes launch; singles: the sum of the members' search launches -- a single handle does not time its
updateNodes launch), the longest member's expansions.  Both sides must give the same results, or the tool stops.
usage: python tools/poly3_lpa_fleet_rate.py [--reps 3] [--sizes 8,64]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpl_ros_amd import poly_map3d as p3  # noqa: E402
from tests import test_poly3_lpa_fleet as T  # noqa: E402


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


def med(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="8,64")
    a = ap.parse_args()
    base = T.acc_members()
    report = {"reps": a.reps, "sizes": {}}
    for N in [int(x) for x in a.sizes.split(",")]:
        members = [base[i % len(base)] for i in range(N)]
        world_of = [int(m[0]) for m in members]
        sides = {"fleet": T.Side(p3.ACC, world_of, fleet=True), "singles": T.Side(p3.ACC, world_of, fleet=False)}
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
                    starts[i][12] = t
        out = {"ticks": []}
        print(f"N={N:3d}  (tick 1 plans afresh; ticks 2..{T.TICKS} repair) wall / kernel ms of updateNodes + plan, medians of {a.reps} repetitions", flush=True)
        for tick in range(T.TICKS):
            row = {"tick": tick + 1, "longest_member_expansions": longest[tick]}
            for k in ("fleet", "singles"):
                wall, kp, ku = zip(*rows[k][tick])
                row[k] = {"wall_ms": med(wall), "plan_kernel_ms": med(kp)}
                if k == "fleet":
                    row[k]["update_kernel_ms"] = med(ku)
            row["wall_ratio_singles_over_fleet"] = row["singles"]["wall_ms"] / row["fleet"]["wall_ms"]
            out["ticks"].append(row)
            print(f"  tick {tick + 1}: longest member {longest[tick]:5d} expansions | fleet wall {row['fleet']['wall_ms']:9.3f}  search kernel {row['fleet']['plan_kernel_ms']:9.3f}"
                  f"  updateNodes kernel {row['fleet']['update_kernel_ms']:7.3f} | singles wall {row['singles']['wall_ms']:9.3f}  search kernels {row['singles']['plan_kernel_ms']:9.3f}"
                  f" | singles / fleet wall {row['wall_ratio_singles_over_fleet']:.2f}", flush=True)
        report["sizes"][str(N)] = out
        del sides
        gc.collect()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
