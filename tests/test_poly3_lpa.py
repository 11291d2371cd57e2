"""-m gpu: LPA* on the 3-D moving-obstacle planner (mplx_plpa3_*, PolyLpa3D): PlannerBase::plan with setLPAstar(true),
PolyMapPlanner<3>::updateNodes and getSubStateSpace in the flow of the replanner node -- every tick the obstacles are where they have
moved to and the planner's start time advances, update_nodes() re-tests every stored predecessor primitive, plan() repairs,
sub_state_space(1) re-roots one primitive ahead.

Everything is compared bit for bit with the Dim-3 LPA* checker (tests/poly_lpa_checker.py; tests/test_poly3_lpa_checker.py pins it to
the compiled reference at Dim 2) after every call: expansion order, every state's g / rhs / h / flags, every predecessor entry with
its blocked bit, the entries updateNodes reports, cost, trajectory."""
import time

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd import poly_map3d as p3
from mpl_ros_amd._capi import MplxError
from tests import poly_lpa_checker as plc
from tests.poly3_scenes import octahedron

pytestmark = pytest.mark.gpu

ACC, JRK = p3.ACC, p3.JRK
KW = {ACC: dict(dt=1.0, v_max=2.0, a_max=1.0, w=10.0), JRK: dict(dt=1.0, v_max=2.0, a_max=1.0, j_max=1.0, w=10.0)}
CASES = [(ACC, False), (ACC, True), (JRK, True)]  # (control, obstacles that change course)
U27 = p3.U27
world, endpoints = p3.replanner_world3, p3.replanner_endpoints3
KEYS = ("states", "g", "rhs", "h", "closed", "opened", "built", "child", "parent", "action", "blocked")
# what a state is keyed on -- ACC: pos3 vel3 t (the checker's Waypoint also carries the control input it arrived with as `acc`); JRK: + acc3
COLS = {ACC: list(range(6)) + [12], JRK: list(range(9)) + [12]}


def same_spaces(sd, so, control, where=""):
    assert sd["initialized"] == so["initialized"], where
    if not so["initialized"]:
        return
    assert sd["n_nodes"] == so["n_nodes"], where
    for k in KEYS:
        a, b = (sd[k][:, COLS[control]], so[k][:, COLS[control]]) if k == "states" else (sd[k], so[k])
        assert np.array_equal(a, b), (where, k)


def compare(K, l, ro, ok, control, where=""):
    """device PolyLpa3D `l` against the checker's state space after the same call sequence: bit-exact"""
    r = l.result
    assert r.status == ro["status"] and ok == (ro["status"] == 0), (where, r.status, ro["status"])
    assert np.array_equal(l.expanded_ids(), ro["expanded"]) and r.n_expanded == len(ro["expanded"]), where
    so, sd = K.lpa_state_space(), l.state_space()
    same_spaces(sd, so, control, where)
    if so["initialized"]:
        assert r.n_nodes == so["n_nodes"], where
    if ro["status"] == 0:
        assert r.cost == ro["cost"], where
        act, ids, st = l.traj()
        assert np.array_equal(act, ro["actions"]) and np.array_equal(ids, ro["node_ids"]), where
        if len(ids):
            assert np.array_equal(st[:, COLS[control]], so["states"][ids][:, COLS[control]]), where


def pair(W, control, U=U27, kw=None, n_worlds=1, at=0):
    """(checker, team, PolyLpa3D) on world W (world `at` of n_worlds copies)"""
    kw = KW[control] if kw is None else kw
    K = plc.LpaCheckerWorld(W, control, U, **kw)
    team = p3.PolyTeam3D()
    team.configure(control, U, **kw)
    team.set_worlds([W] * n_worlds)
    team.set_capacity(1, 1 << 16, 1 << 19, 1 << 19)
    l = team.lpa(at)
    l.set_capacity(1 << 16, 1 << 20, 1 << 20)
    return K, team, l


def both(K, l, control, s, g, where="", **kw):
    ro = K.lpa_plan(s, g, **kw)
    ok = l.plan(s, g, **kw)
    compare(K, l, ro, ok, control, where)
    return ro


def both_update(K, l, where=""):
    uo, ud = K.lpa_update_nodes(), l.update_nodes()
    assert ud == uo, (where, ud[:2], uo[:2])
    return uo


# ---- 4. the replanner flow
@pytest.mark.parametrize("control,turn", CASES)
def test_hip_poly3_lpastar_replays_the_replanner_flow_bit_exact(control, turn):
    K, team, l = pair(world(0.0, turn), control)
    start, goal = endpoints()
    t, blocked, cleared, repairs = 0.0, 0, 0, []
    for tick in range(8):
        W = world(t, turn)
        K.reload(W)
        team.set_worlds([W])
        uo = both_update(K, l, tick)
        blocked += uo[0]; cleared += uo[1]
        ro = both(K, l, control, start, goal, tick)
        # cost == a fresh device A* on the same world (the batched tick planner)
        ra = team.plan_batch([0], [start], [goal], max_expand=-1)[0]
        assert ra.status == l.result.status and ra.cost == l.result.cost, tick
        repairs.append((int(l.result.n_expanded), int(ra.n_expanded), round(l.last_kernel_ms(), 3), round(team.last_kernel_ms(), 3)))
        if ro["status"] != 0 or len(ro["actions"]) <= 2:
            break
        act, ids, st = l.traj()
        K.lpa_sub_state_space(1)
        l.sub_state_space(1)
        same_spaces(l.state_space(), K.lpa_state_space(), control, (tick, "after getSubStateSpace"))
        start = st[1].copy()
        t += 1.0
        start[12] = t
    assert len(repairs) == 8 and cleared > 0 and (blocked > 0 or not turn) and repairs[0][0] == repairs[0][1]
    assert sum(x[0] for x in repairs[1:]) < sum(x[1] for x in repairs[1:])
    print("poly3 LPA* (control=%s turn=%s): (LPA* expansions, fresh A* expansions, LPA* kernel ms, fresh kernel ms) per tick" % (control, turn), repairs)


# ---- 5. the dynamics-aware heuristic
def test_hip_poly3_lpastar_one_tick_pair_with_the_dynamics_aware_heuristic():
    control, turn = ACC, True
    K, team, l = pair(world(0.0, turn), control)
    start, goal = endpoints()
    ro = both(K, l, control, start, goal, "first", heur_ignore_dynamics=False)
    assert ro["status"] == 0 and len(ro["actions"]) > 2
    act, ids, st = l.traj()
    K.lpa_sub_state_space(1)
    l.sub_state_space(1)
    same_spaces(l.state_space(), K.lpa_state_space(), control, "after getSubStateSpace")
    s1 = st[1].copy()
    s1[12] = 1.0
    W = world(1.0, turn)
    K.reload(W)
    team.set_worlds([W])
    uo = both_update(K, l)
    assert uo[0] + uo[1] > 0
    ro = both(K, l, control, s1, goal, "repair", heur_ignore_dynamics=False)
    ra = team.plan_batch([0], [s1], [goal], max_expand=-1, heur_ignore_dynamics=False)[0]
    assert ra.status == l.result.status and ra.cost == l.result.cost


# ---- 6. when the space is kept and when it is not
def test_hip_poly3_lpastar_when_the_space_is_kept_and_when_it_is_not():
    control, turn = ACC, True
    K, team, l = pair(world(0.0, turn), control)
    start, goal = endpoints()
    n0 = len(both(K, l, control, start, goal, "first")["expanded"])
    assert n0 > 50
    goal2 = goal.copy()
    goal2[1] = 4.0
    ro = both(K, l, control, start, goal2, "capped", max_expand=20)   # another goal: a new space; capped after 20 expansions
    assert ro["status"] == 3 and len(ro["expanded"]) == 20
    ro = both(K, l, control, start, goal2, "cap lifted")              # the same call without the cap goes on where the capped one stopped
    assert ro["status"] == 0 and 0 < len(ro["expanded"])
    act, ids, st = l.traj()
    s2 = st[1].copy()
    W = world(1.0, turn)
    K.reload(W)
    team.set_worlds([W])
    both_update(K, l)
    ro = both(K, l, control, s2, goal2, "not the root")               # a start that is not the root (no getSubStateSpace before): a new space
    assert ro["status"] == 0 and l.state_space()["states"][0][12] == 1.0
    both(K, l, control, s2, goal, "first goal again")                 # back to the first goal: a new space again
    K.lpa_reset()
    l.reset()
    assert not l.initialized()
    ro = both(K, l, control, s2, goal, "eps 2", eps=2.0)              # inflated heuristic, from scratch
    assert ro["status"] == 0
    K.lpa_reset()                                                     # a space built under another eps is given up (the checker is told so)
    ro = both(K, l, control, s2, goal, "eps 1 after eps 2")
    assert ro["status"] == 0 and len(ro["expanded"]) > 0
    # mplx_poly3_config after the space was built drops it
    team.configure(control, U27, **KW[control])
    assert l.update_nodes() == (0, 0, []) and not l.initialized()


# ---- 7. all three obstacle kinds, the general solver
def kinds_world(t):
    W = p3.PolyWorld3D((0.0, 0.0, 0.0), (10.0, 8.0, 4.0), start_t=t)
    W.static.append(p3.StaticObstacle3D(octahedron(1.0), (3.0, 4.0, 2.0)))
    W.linear.append(p3.LinearObstacle3D(p3.box(0.6), np.array((6.0, 6.5, 2.0)) + np.array((0.0, -0.7, 0.0)) * t, (0.0, -0.7, 0.0), cov_v=0.15))
    # a jerk trajectory (cubic segments: above degree two) that ends after 4 s and then disappears
    segs = p3.jrk_segs((8.0, 1.0, 1.5), (-0.3, 0.6, 0.0), (0.0, 0.0, 0.0), [(0.2, 0.1, 0.1), (-0.2, -0.1, 0.0), (0.1, 0.2, -0.1), (0.0, -0.2, 0.0)], 1.0)
    W.nonlinear.append(p3.NonlinearObstacle3D(p3.box(0.7), segs, start_t=t, disappear_back=True))
    return W


def test_hip_poly3_lpastar_among_static_linear_and_nonlinear_obstacles():
    control = ACC
    assert np.any(kinds_world(0.0).nonlinear[0].segs[:, [2, 8, 14]] != 0)   # cubic coefficients: the GEN build runs
    K, team, l = pair(kinds_world(0.0), control)
    start = np.zeros(13); start[:3] = (0.5, 4.0, 2.0)
    goal = np.zeros(13); goal[:3] = (9.0, 4.0, 2.0)
    ro = both(K, l, control, start, goal, "first")
    assert ro["status"] == 0 and len(ro["actions"]) > 2
    act, ids, st = l.traj()
    K.lpa_sub_state_space(1)
    l.sub_state_space(1)
    s1 = st[1].copy()
    changes = 0
    for t in (1.0, 2.0):
        W = kinds_world(t)
        K.reload(W)
        team.set_worlds([W])
        uo = both_update(K, l, t)
        changes += uo[0] + uo[1]
        s1[12] = t
        ro = both(K, l, control, s1, goal, ("repair", t))
        if ro["status"] != 0 or len(ro["actions"]) <= 2:
            break
        act, ids, st = l.traj()
        K.lpa_sub_state_space(1)
        l.sub_state_space(1)
        s1 = st[1].copy()
    assert changes > 0


# ---- 8. the world moved and update_nodes was not called
def test_hip_poly3_lpastar_when_the_entries_are_out_of_step_with_the_world():
    control, turn = ACC, True
    K, team, l = pair(world(0.0, turn), control)
    start, goal = endpoints()
    both(K, l, control, start, goal, "first")
    # the world moves on and updateNodes is NOT called: the stored entries are out of step with the obstacles, so a state that is
    # expanded again has to run get_succ again -- as the CPU's loop always does
    W = world(3.0, turn)
    K.reload(W)
    team.set_worlds([W])
    both(K, l, control, start, goal, "moved, no updateNodes")
    uo = both_update(K, l)                                  # ... and now in step again
    assert uo[0] + uo[1] > 0
    ro = both(K, l, control, start, goal, "after updateNodes")
    assert len(ro["expanded"]) > 0
    W = world(4.0, turn)
    K.reload(W)
    team.set_worlds([W])
    both_update(K, l)
    both(K, l, control, start, goal, "next tick")


# ---- 9. lane edges
def open_world():
    return p3.PolyWorld3D((0.0, 0.0, 0.0), (8.0, 6.0, 4.0), start_t=0.0)


def wall_world(t=0.0):
    W = open_world()
    W.start_t = t
    W.linear.append(p3.LinearObstacle3D(p3.box(0.6, 1.2, 1.0), np.array((4.0, 1.0, 2.0)) + np.array((0.0, 0.8, 0.0)) * t, (0.0, 0.8, 0.0), cov_v=0.1))
    return W


U32 = np.concatenate([U27, [(0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.5), (-0.5, 0.0, 0.0), (0.0, -0.5, 0.0)]])
U_TWICE = np.array([(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0)])


@pytest.mark.parametrize("name,U", [("nu_1", np.array([(1.0, 0.0, 0.0)])), ("nu_32", U32), ("two_inputs_one_successor", U_TWICE)])
def test_hip_poly3_lpastar_lane_edges(name, U):
    control = ACC
    kw = dict(dt=1.0, v_max=2.0, a_max=1.0, w=10.0)
    K, team, l = pair(wall_world(0.0), control, U=U, kw=kw)
    start = np.zeros(13); start[:3] = (0.5, 3.0, 2.0)
    goal = np.zeros(13); goal[:3] = (7.0, 3.0, 2.0)
    ro = both(K, l, control, start, goal, "first")
    assert len(ro["expanded"]) > 0
    if name == "two_inputs_one_successor":
        so = K.lpa_state_space()
        first = so["parent"] == 0
        assert len(set(so["child"][first].tolist())) < int(first.sum())   # two entries of the first expansion lead to one state
    W = wall_world(1.0)
    K.reload(W)
    team.set_worlds([W])
    both_update(K, l)
    both(K, l, control, start, goal, "repair")


def test_hip_poly3_lpastar_in_a_world_with_no_obstacle():
    control = ACC
    K, team, l = pair(open_world(), control)
    start = np.zeros(13); start[:3] = (0.5, 3.0, 2.0)
    goal = np.zeros(13); goal[:3] = (7.0, 3.0, 2.0)
    ro = both(K, l, control, start, goal, "first")
    assert ro["status"] == 0
    assert both_update(K, l) == (0, 0, [])
    assert len(both(K, l, control, start, goal, "again")["expanded"]) == 0


# ---- 10. degenerate outcomes
def test_hip_poly3_lpastar_degenerate_outcomes():
    control = ACC
    K, team, l = pair(wall_world(0.0), control)
    goal = np.zeros(13); goal[:3] = (7.0, 3.0, 2.0)
    outside = np.zeros(13); outside[:3] = (0.5, 3.0, 4.5)
    ro = both(K, l, control, outside, goal, "start outside the bounding box")
    assert ro["status"] == 2 and not l.initialized() and l.result.n_expanded == 0
    at_goal = goal.copy(); at_goal[0] -= 0.25
    ro = both(K, l, control, at_goal, goal, "start inside the goal tolerance")
    assert ro["status"] == 0 and ro["cost"] == 0 and l.result.n_expanded == 0 and not l.initialized()
    # a sealed start: a standing box around it that every primitive leaves through
    W = open_world()
    W.static.append(p3.StaticObstacle3D(p3.box(0.4), (0.5, 3.0, 2.0)))
    K2, team2, l2 = pair(W, control)
    start = np.zeros(13); start[:3] = (0.5, 3.0, 2.0)
    ro = both(K2, l2, control, start, goal, "sealed start")
    assert ro["status"] == 1 and len(ro["expanded"]) >= 1
    # pools too small (one chunk each: 32 768 states, 65 536 entries), then large enough: a longer way through the replanner world
    K3, team3, l3 = pair(world(0.0, False), ACC)
    s3, g3 = endpoints()
    s3[0], g3[0] = 0.5, 16.0
    l3.set_capacity(1 << 10, 1 << 12, 1 << 12)
    assert not l3.plan(s3, g3) and l3.result.status == _capi.PLAN_POOL_FULL and not l3.initialized()
    l3.set_capacity(1 << 19, 1 << 22, 1 << 21)
    ro = both(K3, l3, ACC, s3, g3, "after a larger set_capacity")
    assert ro["status"] == 0 and K3.lpa_state_space()["n_nodes"] > (1 << 15)


# ---- 11. two planners on one team
def test_hip_poly3_lpastar_two_planners_on_one_team_in_different_worlds():
    control = ACC
    Wa, Wb = world(0.0, False), wall_world(0.0)
    Ka = plc.LpaCheckerWorld(Wa, control, U27, **KW[control])
    Kb = plc.LpaCheckerWorld(Wb, control, U27, **KW[control])
    team = p3.PolyTeam3D()
    team.configure(control, U27, **KW[control])
    team.set_worlds([Wa, Wb])
    team.set_capacity(2, 1 << 16, 1 << 19, 1 << 19)
    la, lb = team.lpa(0), team.lpa(1)
    for l in (la, lb):
        l.set_capacity(1 << 16, 1 << 20, 1 << 20)
    sa, ga = endpoints()
    sb = np.zeros(13); sb[:3] = (0.5, 3.0, 2.0)
    gb = np.zeros(13); gb[:3] = (7.0, 3.0, 2.0)
    both(Ka, la, control, sa, ga, "a first")
    both(Kb, lb, control, sb, gb, "b first")
    ra, rb = team.plan_batch([0, 1], [sa, sb], [ga, gb], max_expand=-1)
    assert ra.cost == la.result.cost and rb.cost == lb.result.cost
    Wa, Wb = world(1.0, False), wall_world(1.0)
    Ka.reload(Wa); Kb.reload(Wb)
    team.set_worlds([Wa, Wb])
    both_update(Kb, lb, "b")
    team.plan_batch([1, 0], [sb, sa], [gb, ga], max_expand=-1)
    both_update(Ka, la, "a")
    both(Kb, lb, control, sb, gb, "b repair")
    team.plan_batch([0], [sa], [ga], max_expand=-1)
    both(Ka, la, control, sa, ga, "a repair")


# ---- 12. refusals
def test_hip_poly3_lpastar_refusals():
    start, goal = endpoints()
    team = p3.PolyTeam3D()
    l = team.lpa()
    with pytest.raises(MplxError, match="mplx error %d: .*config" % _capi.ERR_ARG):     # not configured
        l.plan(start, goal)
    team.configure(ACC, U27, **KW[ACC])
    with pytest.raises(MplxError, match="mplx error %d: .*commit" % _capi.ERR_ARG):     # not committed
        l.plan(start, goal)
    team.set_worlds([world(0.0)])
    with pytest.raises(MplxError, match="mplx error %d: .*world index" % _capi.ERR_ARG):
        team.lpa(1).plan(start, goal)
    with pytest.raises(MplxError, match="mplx error %d: .*world index" % _capi.ERR_ARG):
        team.lpa(-1).update_nodes()
    team.configure(p3.VEL, U27, **KW[ACC])
    team.set_worlds([world(0.0)])
    with pytest.raises(MplxError, match="mplx error %d: .*ACC or JRK" % _capi.ERR_ARG):
        l.plan(start, goal)
    assert l.result is None and not l.initialized() and l.last_kernel_ms() == 0.0    # nothing was launched
    team.configure(ACC, U27, **KW[ACC])
    assert l.plan(start, goal)


# ---- 13. the launch deadline
def test_hip_poly3_lpastar_honours_the_launch_deadline():
    control = ACC
    K, team, l = pair(world(0.0, False), control)
    start, goal = endpoints()
    ro = both(K, l, control, start, goal, "first")
    assert len(ro["expanded"]) > 1000
    ms = l.last_kernel_ms()
    l.reset()
    team.set_deadline(ms / 1000.0 / 50.0)
    t0 = time.time()
    with pytest.raises(MplxError, match="mplx error %d: .*aborted" % _capi.ERR_TIMEOUT):
        l.plan(start, goal)
    assert time.time() - t0 < 10.0 and not l.initialized()
    team.set_deadline(60.0)
    K.lpa_reset()                                            # (the aborted launch left no space: the same plan from scratch, bit for bit)
    both(K, l, control, start, goal, "after the timeout")
