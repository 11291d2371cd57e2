"""The bit-exact comparison bodies of the moving-obstacle tests, 2-D (tests/test_poly_map.py, tests/test_poly_geometry.py) and
3-D (tests/test_poly_map3d.py, tests/test_poly3_geometry.py): the device's get_succ_batch / plan_batch against a CPU
environment -- refpoly.RefWorld / RefWorld3D (the compiled reference) or tests/poly_checker.CheckerWorld; all of them have
get_succ(state), plan(start, goal, ...) and node(id) -> (state, ...).  States are pos vel acc jrk (dim each) t.
TEST INFRASTRUCTURE ONLY."""
import numpy as np


def same_succ(a, b):
    """two CPU environments on one state: (succ, cost, action) bit for bit, the signs of zero too, inf matched to inf"""
    (sa, ca, aa), (sb, cb, ab) = a, b
    assert np.array_equal(aa, ab)
    assert np.array_equal(sa, sb)  # bit-exact f64 (array_equal: -0.0 == 0.0, the sign is checked below)
    assert np.array_equal(np.signbit(sa), np.signbit(sb))
    assert all(x == y or (np.isinf(x) and np.isinf(y)) for x, y in zip(ca, cb))
    return int(np.isinf(ca).sum()), int(np.isfinite(ca).sum())


def path_cols(dim, compare_acc):
    """position, velocity (JRK states: acceleration too) and time of a state of that dimension"""
    return list(range((3 if compare_acc else 2) * dim)) + [4 * dim]


def same_plan(a, b, ref, chk, cols):
    """two CPU environments on one plan: status, expansion order, node count, cost, actions, node ids and path states"""
    assert a["status"] == b["status"]
    assert np.array_equal(a["expanded"], b["expanded"]) and a["n_nodes"] == b["n_nodes"]
    assert a["cost"] == b["cost"] or (np.isinf(a["cost"]) and np.isinf(b["cost"]))
    assert np.array_equal(a["actions"], b["actions"]) and np.array_equal(a["node_ids"], b["node_ids"])
    for nid in a["node_ids"]:
        assert np.array_equal(ref.node(int(nid))[0][cols], chk.node(int(nid))[0][cols])


def compare_get_succ(team, worlds, refs, world_of, states, n_u, signs=False):
    """signs: the sign of every zero of a successor state must agree too (array_equal takes -0.0 for 0.0)"""
    out = team.get_succ_batch(world_of, states)
    n_inf = n_fin = 0
    for k, (w, s) in enumerate(zip(world_of, states)):
        succ, cost, act = refs[w].get_succ(s)
        got = [out[k * n_u + i] for i in range(n_u)]
        gv = [g for g in got if g.valid]
        assert [g.action for g in gv] == act.tolist(), (k, w)
        for g, so, co in zip(gv, succ, cost):
            assert np.array_equal(np.array(g.state[:]), so), (k, g.action)        # bit-exact f64
            if signs:
                assert np.array_equal(np.signbit(np.array(g.state[:])), np.signbit(so)), (k, g.action)
            assert g.cost == co or (np.isinf(g.cost) and np.isinf(co)), (k, g.action, g.cost, co)
            n_inf += int(np.isinf(co)); n_fin += int(np.isfinite(co))
    return n_fin, n_inf


def compare_plans(team, refs, world_of, starts, goals, compare_acc=False, dim=2, **kw):
    """kw: the plan parameters, given to the device and to the CPU environment alike (tol_vel only where it is named: the
    compiled reference's search has the position test only)"""
    cols = path_cols(dim, compare_acc)  # (JRK states carry their acceleration)
    team.set_record(1 << 16)
    R = team.plan_batch(world_of, starts, goals, **kw)
    n_ok = 0
    for k, w in enumerate(world_of):
        extra = dict(tol_vel=kw["tol_vel"]) if "tol_vel" in kw else {}
        ref = refs[w].plan(starts[k], goals[k], eps=kw.get("eps", 1.0), tol_pos=kw.get("tol_pos", 0.5), max_expand=kw.get("max_expand", -1),
                           heur_ignore_dynamics=kw.get("heur_ignore_dynamics", True), **extra)
        r = R[k]
        assert r.status == ref["status"], (k, r.status, ref["status"])
        assert r.n_expanded == len(ref["expanded"]) and r.n_nodes == ref["n_nodes"], (k, r.n_expanded, len(ref["expanded"]), r.n_nodes, ref["n_nodes"])
        assert np.array_equal(team.expanded_ids(k), ref["expanded"]), k  # same nodes in the same order
        if ref["status"] == 0:
            n_ok += 1
            assert r.cost == ref["cost"], (k, r.cost, ref["cost"])  # bit-exact f64
            act, ids, st = team.traj(k)
            assert np.array_equal(act, ref["actions"]) and np.array_equal(ids, ref["node_ids"]), k
            for i, nid in enumerate(ids):  # waypoint states: position, velocity and time of every node of the path
                s = refs[w].node(int(nid))[0]
                assert np.array_equal(st[i][cols], s[cols]), (k, i)
        else:
            assert np.isinf(r.cost)
    return R, n_ok
