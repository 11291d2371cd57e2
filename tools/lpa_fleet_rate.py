"""Numbers of the LPA* fleet (no gate): the repairs of N robots on one shared map as N single-planner calls one after the other
against one fleet call.  BASELINE C2 size: mapgen.benchmark_map(256), the 27-input lattice, the capacities of benchmarks/lpa.py;
N = 1, 16, 64 members with pairs from mapgen.c4_queries on that map (the first N whose first plan finds a path), one 5^3 box on
the middle of every member's first path.  Per N, in one process, alternated and repeated --reps times:
  (a) updateBlockedNodes + plan of N VoxelMapPlanner(setLPAstar(True)) one after the other,
  (b) updateBlockedNodes + plan of an LpaFleet of N
(the boxes are removed again between the repetitions, with updateClearedNodes + plan on both sides).  Wall ms and kernel ms per
leg with their spread, the longest member's expansions, and -- a restatement on ONE core, not the device's competitor -- the CPU
checker's single-thread time for the same N repairs (--cpu).  Leg (a) uses only calls older builds have: on a build without the
fleet entry points leg (b) is skipped, which gives that build's figure from the same script.
usage: python tools/lpa_fleet_rate.py [--reps 10] [--sizes 1,16,64] [--cpu]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpl_ros_amd import mapgen, planner  # noqa: E402
from mpl_ros_amd.planner import ACC, VoxelMapPlanner, VoxelMapUtil, Waypoint3D  # noqa: E402

CAP = (1 << 19, 1 << 21, 1 << 22)  # benchmarks/lpa.py


def wp(p, v=(0, 0, 0)):
    w = Waypoint3D(ACC)
    w.pos, w.vel = np.array(p, dtype=np.float64), np.array(v, dtype=np.float64)
    return w


def setup(pl, U):
    pl.setVmax(2.0); pl.setAmax(1.0); pl.setDt(1.0); pl.setU(U); pl.setTol(0.5)
    pl.setCapacity(1, *CAP)
    return pl


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="1,16,64")
    ap.add_argument("--cpu", action="store_true", help="also time the CPU checker's LPA* (one thread) on the same repairs")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    n_max = max(sizes)
    have_fleet = hasattr(planner, "LpaFleet")
    n = 256
    grid, origin, res, _, _, _ = mapgen.benchmark_map(n)
    U = mapgen.control_lattice(1.0, 1, True)
    mu = VoxelMapUtil(0)

    def set_map(g):
        dz, dy, dx = g.shape
        mu.setMap(origin, (dx, dy, dz), g.ravel(), res)

    def single():
        pl = VoxelMapPlanner(False)
        pl.setMapUtil(mu)
        setup(pl, U)
        pl.setLPAstar(True)
        return pl

    def box_on(center, half=2):
        c = [int(round((center[i] - origin[i]) / res - 0.5)) for i in range(3)]  # MapUtil::floatToInt
        return [(c[0] + dx, c[1] + dy, c[2] + dz) for dz in range(-half, half + 1) for dy in range(-half, half + 1) for dx in range(-half, half + 1)
                if 0 <= c[0] + dx < n and 0 <= c[1] + dy < n and 0 <= c[2] + dz < n and grid[c[2] + dz, c[1] + dy, c[0] + dx] == 0]

    # the members: the first n_max pairs of the C4 stream whose first plan finds a path within the capacities
    set_map(grid)
    singles, pairs, mids, first_exp = [], [], [], []
    for s, g in mapgen.c4_queries(grid, origin, res, 4 * n_max):
        pl = single()
        if pl.plan(wp(s), wp(g)):
            w = pl.getTraj().getWaypoints()
            singles.append(pl); pairs.append((tuple(s), tuple(g))); mids.append(tuple(w[len(w) // 2].pos)); first_exp.append(int(pl.getResult().n_expanded))
            if len(pairs) == n_max:
                break
        else:
            del pl
    assert len(pairs) == n_max, f"only {len(pairs)} of {n_max} members found a path"
    print(f"# {n_max} members; first plans expand {min(first_exp)} ... {max(first_exp)} states; fleet entry points: {'yes' if have_fleet else 'no (leg b skipped)'}", flush=True)
    report = {"reps": a.reps, "first_plan_expansions": first_exp, "sizes": {}}

    checkers = []
    if a.cpu:
        from oracle import orc
        from tests import util
        for s, g in pairs:
            L = util.make_oracle(grid, origin, res, orc.ACC, U, v_max=2.0, a_max=1.0, tol_pos=0.5)
            L.set_lpastar(True)
            assert L.plan(orc.waypoint(s), orc.waypoint(g)) == orc.OK
            checkers.append(L)

    for N in sizes:
        S = [wp(s) for s, _ in pairs[:N]]
        G = [wp(g) for _, g in pairs[:N]]
        cells = sorted(set(c for m in mids[:N] for c in box_on(m)))
        g2 = grid.copy()
        for x, y, z in cells:
            g2[z, y, x] = 100
        fleet = None
        if have_fleet:
            fleet = setup(planner.LpaFleet(mu, N), U)
            set_map(grid)
            r = fleet.plan(S, G)
            assert all(x.status == 0 for x in r) and fleet.stats() == [0, 0, N, 0]

        def leg_a(update):
            t0 = time.perf_counter()
            for pl in singles[:N]:
                update(pl)
            t1 = time.perf_counter()
            k = 0.0
            for i, pl in enumerate(singles[:N]):
                pl.plan(S[i], G[i])  # (a member the boxes cut off reports no path on both sides)
                k += pl.lastKernelMs()
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, k, [pl.getResult() for pl in singles[:N]]

        def leg_b(update):
            t0 = time.perf_counter()
            update(fleet)
            t1 = time.perf_counter()
            r = fleet.plan(S, G)
            t2 = time.perf_counter()
            assert fleet.stats() == [N, 1, 0, 0]
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, fleet.lastKernelMs()[0], r

        rows = {"a": [], "b": []}
        exp = None
        for rep in range(a.reps + 1):  # (the first repetition warms up and is not counted)
            set_map(g2)
            order = ("a", "b") if rep % 2 == 0 else ("b", "a")
            got = {}
            for leg in order:
                if leg == "a":
                    got["a"] = leg_a(lambda pl: pl.updateBlockedNodes(cells))
                elif fleet is not None:
                    got["b"] = leg_b(lambda f: f.updateBlockedNodes(cells))
            if "b" in got:  # the same searches on both sides
                for x, y in zip(got["a"][3], got["b"][3]):
                    assert (x.cost, x.n_expanded, x.expand_hash) == (y.cost, y.n_expanded, y.expand_hash)
            exp = [int(x.n_expanded) for x in got["a"][3]]
            if rep > 0:
                for k, v in got.items():
                    rows[k].append(v[:3])
            set_map(grid)
            leg_a(lambda pl: pl.updateClearedNodes(cells))
            if fleet is not None:
                leg_b(lambda f: f.updateClearedNodes(cells))
        out = {"cells": len(cells), "repair_expansions": exp, "longest_member_expansions": max(exp), "sum_expansions": sum(exp)}
        for k, name in (("a", "sequential_singles"), ("b", "fleet")):
            if rows[k]:
                u, w, ker = zip(*rows[k])
                out[name] = {"update_wall_ms": spread(u), "plan_wall_ms": spread(w), "plan_kernel_ms": spread(ker)}
        if "fleet" in out:
            A, B = out["sequential_singles"], out["fleet"]
            out["plan_wall_ratio_singles_over_fleet"] = A["plan_wall_ms"]["median"] / B["plan_wall_ms"]["median"]
            out["update_wall_ratio_singles_over_fleet"] = A["update_wall_ms"]["median"] / B["update_wall_ms"]["median"]
        if checkers:
            from oracle import orc
            for L in checkers[:N]:
                L.set_map(g2, origin, res)
                L.update_blocked(cells)
            t0 = time.perf_counter()
            for i, L in enumerate(checkers[:N]):
                L.reset_counters()
                L.plan(orc.waypoint(pairs[i][0]), orc.waypoint(pairs[i][1]))
            out["cpu_checker_one_thread_ms"] = (time.perf_counter() - t0) * 1e3
            out["cpu_checker_expansions"] = [int(L.lpa_iterations()) for L in checkers[:N]]
            for i, L in enumerate(checkers[:N]):  # back to the first map for the next N
                L.set_map(grid, origin, res)
                L.update_cleared(cells)
                L.plan(orc.waypoint(pairs[i][0]), orc.waypoint(pairs[i][1]))
        report["sizes"][str(N)] = out
        line = f"N={N:3d} cells {len(cells):5d} longest member {max(exp)} expansions (sum {sum(exp)})"
        for name in ("sequential_singles", "fleet"):
            if name in out:
                o = out[name]
                line += (f"\n    {name:18s} plan wall {o['plan_wall_ms']['median']:8.3f} ms [{o['plan_wall_ms']['min']:.3f} .. {o['plan_wall_ms']['max']:.3f}]"
                         f"  kernel {o['plan_kernel_ms']['median']:8.3f} ms [{o['plan_kernel_ms']['min']:.3f} .. {o['plan_kernel_ms']['max']:.3f}]"
                         f"  update wall {o['update_wall_ms']['median']:8.3f} ms [{o['update_wall_ms']['min']:.3f} .. {o['update_wall_ms']['max']:.3f}]")
        if "cpu_checker_one_thread_ms" in out:
            line += f"\n    CPU checker, one thread (a restatement, one core): {out['cpu_checker_one_thread_ms']:.3f} ms for the same {N} repairs"
        print(line, flush=True)
        del fleet
        gc.collect()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
