"""Numbers of the point-cloud planner (no gate): kernel time of the office-shaped query with the launch file's parameters,
expansions per second of a 64-query batch on the same cloud, point tests per expansion, and the CPU checker's
single-thread time for the same query.  usage: python tools/cloud_rate.py [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd.ellipsoid import ACC, EllipsoidPlanner, control_lattice, state13  # noqa: E402
from tests import cloud_scenes as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-checker", action="store_true")
    a = ap.parse_args()
    L = S.LAUNCH
    pts = S.office()
    U = control_lattice(L["u_max"], L["num"], False)
    pl = EllipsoidPlanner(False)
    pl.set_map(pts, L["r"], S.ORI, S.DIM)
    pl.set_control(ACC)
    pl.set_u(U)
    pl.set_dt(L["dt"]); pl.set_vmax(L["v_max"]); pl.set_amax(L["a_max"]); pl.set_w(L["w"])
    pl.set_epsilon(L["eps"]); pl.set_tol(*L["tol"])
    start, goal = state13(S.START), state13(S.GOAL)
    pl.plan(start, goal)  # warm-up
    ms = []
    for _ in range(a.reps):
        pl.plan(start, goal)
        ms.append(pl.last_kernel_ms())
    r = pl.result()
    out = {"points": int(len(pts)), "single_status": r["status"], "single_cost": r["cost"], "single_expanded": r["n_expanded"],
           "single_kernel_ms_median": float(np.median(ms)), "point_tests_per_expansion": r["voxel_reads"] / max(1, r["n_expanded"])}
    rng = np.random.default_rng(64)
    xs = [7.5, 10.0, 14.0, 16.0, 20.0, 22.0, 26.0, 29.5]
    starts, goals = [], []
    for _ in range(64):
        i, j = rng.choice(len(xs), 2, replace=False)
        starts.append(state13((xs[i], rng.uniform(13.0, 16.0), 1.3)))
        goals.append(state13((xs[j], rng.uniform(13.0, 16.0), 1.3)))
    pl.set_max_num(3000)
    pl.plan_batch(starts, goals)
    bms = []
    for _ in range(a.reps):
        res = pl.plan_batch(starts, goals)
        bms.append(pl.last_kernel_ms())
    exp = sum(x["n_expanded"] for x in res)
    out.update(batch_queries=64, batch_expanded=exp, batch_kernel_ms_median=float(np.median(bms)),
               batch_expansions_per_s=exp / (float(np.median(bms)) / 1e3), batch_ok=sum(x["status"] == 0 for x in res),
               batch_point_tests_per_expansion=sum(x["voxel_reads"] for x in res) / max(1, exp))
    if not a.no_checker:
        from tests import cloud_checker as K
        ck = K.Checker(K.Cloud(pts, L["r"], S.ORI, S.DIM), ACC, U, L["dt"], v_max=L["v_max"], a_max=L["a_max"], w=L["w"])
        t0 = time.perf_counter()
        c = ck.plan(start, goal, eps=L["eps"], tol_pos=L["tol"][0], tol_vel=L["tol"][1], tol_acc=L["tol"][2])
        out.update(checker_single_s=time.perf_counter() - t0, checker_expanded=len(c["expanded"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
