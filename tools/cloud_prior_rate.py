"""Numbers of the prior-guided point-cloud search (no gate), on the scene of tools/cloud_rate.py: a JRK and an SNP query, each
run once alone and once guided by the ACC plan of the same query (setPriorTrajectory: the hierarchical refinement of
ellipsoid_planner_node.cpp:121-139), with expansions and kernel time; and a batch of 64 such pairs in one launch each way.
usage: python tools/cloud_prior_rate.py [--reps N] [--max-num N]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd.ellipsoid import ACC, JRK, SNP, EllipsoidPlanner, control_lattice, prior_from_traj, state13  # noqa: E402
from tests import cloud_scenes as S  # noqa: E402


def planner(control, max_num):
    L = S.LAUNCH
    pl = EllipsoidPlanner(False)
    pl.set_map(S.office(), L["r"], S.ORI, S.DIM)
    pl.set_control(control)
    pl.set_u(control_lattice(L["u_max"], L["num"], False))
    pl.set_dt(L["dt"]); pl.set_vmax(L["v_max"]); pl.set_amax(L["a_max"]); pl.set_w(L["w"])
    pl.set_epsilon(L["eps"]); pl.set_tol(*L["tol"])
    pl.set_max_num(max_num)
    return pl


def acc_priors(starts, goals, max_num):
    """the ACC plan of every query, sampled with the dt and w in force (P1); None where the ACC search found no plan"""
    L = S.LAUNCH
    pl = planner(ACC, max_num)
    pl.set_capacity(len(starts), 1 << 21, 1 << 23, 1 << 22)
    res = pl.plan_batch(starts, goals)
    ms = pl.last_kernel_ms()
    priors = []
    for q in range(len(starts)):
        tr = pl.get_traj(q)
        priors.append(None if tr is None else prior_from_traj(tr["states"], tr["actions"], pl.U, ACC, L["dt"], L["w"]))
    return priors, ms, sum(r["n_expanded"] for r in res)


def timed(pl, starts, goals, priors, reps):
    pl.plan_batch(starts, goals, priors=priors)  # warm-up
    ms = []
    for _ in range(reps):
        res = pl.plan_batch(starts, goals, priors=priors)
        ms.append(pl.last_kernel_ms())
    return res, float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-num", type=int, default=20000)
    a = ap.parse_args()
    out = {"max_num": a.max_num}
    start, goal = [state13(S.START)], [state13(S.GOAL)]
    p1, ms_acc, exp_acc = acc_priors(start, goal, a.max_num)
    out.update(acc_expanded=exp_acc, acc_kernel_ms=ms_acc, prior_entries=0 if p1[0] is None else int(len(p1[0]["cost_to_go"])))
    rng = np.random.default_rng(64)
    xs = [7.5, 10.0, 14.0, 16.0, 20.0, 22.0, 26.0, 29.5]
    starts, goals = [], []
    for _ in range(64):
        i, j = rng.choice(len(xs), 2, replace=False)
        starts.append(state13((xs[i], rng.uniform(13.0, 16.0), 1.3)))
        goals.append(state13((xs[j], rng.uniform(13.0, 16.0), 1.3)))
    p64, ms_acc64, exp_acc64 = acc_priors(starts, goals, 3000)
    out.update(batch_queries=64, batch_priors=sum(p is not None for p in p64), batch_acc_expanded=exp_acc64, batch_acc_kernel_ms=ms_acc64)
    for name, control in (("jrk", JRK), ("snp", SNP)):
        pl = planner(control, a.max_num)
        pl.set_capacity(1, 1 << 21, 1 << 23, 1 << 22)
        for tag, pr in (("alone", None), ("guided", p1)):  # (alone: no prior in force, the plain search kernel)
            res, ms = timed(pl, start, goal, pr, a.reps)
            out.update({f"{name}_{tag}_status": res[0]["status"], f"{name}_{tag}_cost": res[0]["cost"], f"{name}_{tag}_expanded": res[0]["n_expanded"],
                        f"{name}_{tag}_reopened": res[0]["n_reopen"], f"{name}_{tag}_kernel_ms": ms})
        pb = planner(control, 3000)
        pb.set_capacity(64, 1 << 22, 1 << 24, 1 << 23)
        for tag, pr in (("alone", None), ("guided", p64)):
            res, ms = timed(pb, starts, goals, pr, a.reps)
            out.update({f"{name}_batch_{tag}_ok": sum(r["status"] == 0 for r in res), f"{name}_batch_{tag}_expanded": sum(r["n_expanded"] for r in res),
                        f"{name}_batch_{tag}_kernel_ms": ms})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
