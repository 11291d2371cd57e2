"""The two comparisons every GPU test of the point-cloud planner goes through, bit for bit against the CPU checker
(tests/cloud_checker.py): env_cloud::get_succ of a batch of states, and one plan with its expansion order, state space and
trajectory.  `pl` is an EllipsoidPlanner, `ck` a cloud_checker.Checker on the same cloud and settings; a plan runs with the
launch file's epsilon and tolerances (cloud_scenes.LAUNCH), which the caller has set on `pl`."""
import math

import numpy as np

from tests import cloud_checker as K
from tests import cloud_scenes as S

L = S.LAUNCH


def _compare_succ(pl, ck, states):
    valid, succ, cost, act = pl.get_succ_batch(states)
    for k, s13 in enumerate(states):
        for i, (ok, st, c, a) in enumerate(ck.get_succ(s13)):
            assert bool(valid[k, i]) == ok, (k, i)
            assert act[k, i] == a
            assert np.array_equal(succ[k, i], st), (k, i, succ[k, i], st)
            assert (math.isinf(c) and math.isinf(cost[k, i])) or cost[k, i] == c, (k, i)
    return int(valid.sum())


def _compare_plan(pl, ck, start, goal, max_num=-1):
    pl.set_max_num(max_num)
    pl.set_record(1 << 16)
    ok = pl.plan(start, goal)
    r = pl.result()
    c = ck.plan(start, goal, eps=L["eps"], tol_pos=L["tol"][0], tol_vel=L["tol"][1], tol_acc=L["tol"][2], max_num=max_num)
    assert r["status"] == c["status"]
    assert r["n_expanded"] == len(c["expanded"])
    assert list(pl.expanded_ids()) == c["expanded"]
    assert r["expand_hash"] == K.expand_hash(c["expanded"])
    assert r["n_nodes"] == len(c["states"])
    st, g, closed, opened = pl.nodes()
    assert sorted(map(tuple, st[closed, :3])) == sorted(tuple(s[:3]) for s, cl in zip(c["states"], c["closed"]) if cl)
    assert np.array_equal(st, np.array(c["states"]))
    if ok:
        assert r["cost"] == c["cost"]
        tr = pl.get_traj()
        assert np.array_equal(tr["states"], c["traj"]["states"])
        assert tr["actions"].tolist() == c["traj"]["actions"]
    assert len(pl.get_expanded_nodes()) == 0
    return r, c
