"""Fleets of 3-D moving-obstacle LPA* planners (mplx_plpa3_fleet_*, poly_map3d.PolyLpaFleet3D): N PolyLpa3D planners on one PolyTeam3D
whose plan(), update_nodes() and sub_state_space() run for all members in one launch each.  Per member every result must be what the
same sequence of single-handle calls gives, bit for bit -- the standard of tests/test_poly3_lpa.py, whose compare / same_spaces / KW /
COLS / KEYS are used here: after every call every member equals the Dim-3 LPA* checker (tests/poly_lpa_checker.LpaCheckerWorld, ONE
LIVE INSTANCE PER MEMBER, driven in step with the device) in expansion order, every state's g / rhs / h / flags, every predecessor
entry with its blocked bit, the entries updateNodes reports, cost and trajectory.

World: p3.replanner_world3(t, turn); world 0 is turn=False, world 1 is turn=True (they differ from t = 2 on).  Lattice U27, cap 5 000
expansions, capacity per member (2^15, 2^18, 2^18).  The flow, five ticks (ticks 3 to 5 see the two worlds apart): commit both worlds
at t, update_nodes, plan, sub_state_space(1), go on from the second state of the trajectory with t += 1.

CPU: the checker facts the GPU tests rest on; the library exports the fleet; null handles; the C++ driver compiles and fails loudly
without a GPU.  GPU: fleet against a checker per member, fleet against N single handles, JRK (the GEN build), a mixed call, pool
exhaustion, trust_entries, the driver."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd import poly_map3d as p3
from tests import poly_lpa_checker as plc
from tests.test_poly3_lpa import COLS, KEYS, KW, compare, same_spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mpl_ros_amd", "csrc")
ACC, JRK = p3.ACC, p3.JRK
U27 = p3.U27
TICKS = 5
MAX_EXPAND = 5000
CAP = (1 << 15, 1 << 18, 1 << 18)  # states, entries, OPEN-log records per member
BIG_CAP = (1 << 17, 1 << 20, 1 << 20)
# position start -> goal; velocity and acceleration zero
ACC_PAIRS = [((4, 10, 2), (19, 10, 2)), ((5, 2, 2), (12, 18, 2)), ((2, 9, 1), (15, 9, 3)), ((9, 2, 3), (9, 18, 1))]
JRK_PAIR = ((4, 10, 2), (19, 10, 2))
CAPPED_PAIRS = [((3, 4, 1), (17, 15, 3)), ((16, 17, 1), (4, 5, 3))]  # the first plan runs into the cap of 5 000 expansions
BIG_PAIR = ((18, 12, 2), (3, 8, 2))                                   # with the cap lifted: more than 2^15 states
# what the checker gives for the first plan of the pairs above at t = 0 with the cap lifted: (expansions, states)
FIRST_PLANS = {ACC: [(2222, 13159), (940, 7049), (3831, 20236), (1717, 11371)], JRK: [(2431, 14582)]}
FLEET_NAMES = ["mplx_plpa3_fleet_create", "mplx_plpa3_fleet_destroy", "mplx_plpa3_fleet_last_error", "mplx_plpa3_fleet_size", "mplx_plpa3_fleet_member",
               "mplx_plpa3_fleet_set_capacity", "mplx_plpa3_fleet_set_world", "mplx_plpa3_fleet_plan", "mplx_plpa3_fleet_update_nodes",
               "mplx_plpa3_fleet_sub_state_space", "mplx_plpa3_fleet_stats", "mplx_plpa3_fleet_last_kernel_ms"]


def state13(p, t=0.0):
    s = np.zeros(13)
    s[0:3], s[12] = p, t
    return s


def members_of(pairs):
    """(turn, start, goal) per pair and world -- member i lives in world int(turn)"""
    return [(turn, state13(s), state13(g)) for s, g in pairs for turn in (False, True)]


def acc_members():
    return members_of(ACC_PAIRS)


def jrk_members():
    return members_of([JRK_PAIR])


def worlds(t):
    return [p3.replanner_world3(t, False), p3.replanner_world3(t, True)]


def checker(control, turn, t=0.0):
    return plc.LpaCheckerWorld(p3.replanner_world3(t, turn), control, U27, **KW[control])


# ---------------------------------------------------------------------------------------------------------------- CPU
def checker_flow(control, member, recommit=()):
    """The flow of one member on the checker alone: per tick dict(upd, plan, n_nodes, astar) -- astar: the checker's fresh best-first
    search from the same start through the same world: (status, cost).  recommit: as in run_flow."""
    turn, start, goal = member
    K, A = checker(control, turn), checker(control, turn)
    start, t, recs = start.copy(), 0.0, []
    for tick in range(TICKS):
        W = p3.replanner_world3(t, turn)
        K.reload(W)
        upd = K.lpa_update_nodes()
        if tick in recommit:
            K.reload(p3.replanner_world3(t, not turn))
        ro = K.lpa_plan(start, goal, max_expand=MAX_EXPAND)
        A.reload(W)
        ra = A.plan(start, goal, max_expand=-1)
        ss = K.lpa_state_space()
        recs.append(dict(upd=upd, plan=ro, n_nodes=ss["n_nodes"], astar=(ra["status"], ra["cost"])))
        if ro["status"] != 0 or len(ro["actions"]) <= 2:
            break
        K.lpa_sub_state_space(1)
        start = ss["states"][ro["node_ids"][1]].copy()
        t += 1.0
        start[12] = t
    return recs


def test_checker_facts_of_the_members():
    """Conditions on the INPUTS of the GPU tests (not measurements of the device), re-derived from the checker: every flow member
    completes the five ticks with status 0, its LPA* cost equals the checker's fresh best-first search at every tick, updateNodes
    reports changed entries, at least one of its repairs expands a state, its largest space fits CAP; the first plans are the ones
    the members were chosen by; the capped pairs stop at exactly 5 000 expansions with a space that fits CAP; the pool-full pair needs
    more than CAP and fits BIG_CAP."""
    for control, members in ((ACC, acc_members()), (JRK, jrk_members())):
        for k, m in enumerate(members):
            recs = checker_flow(control, m)
            assert len(recs) == TICKS and all(r["plan"]["status"] == 0 for r in recs), (control, k, [r["plan"]["status"] for r in recs])
            for tick, r in enumerate(recs):
                assert (r["plan"]["status"], r["plan"]["cost"]) == r["astar"], (control, k, tick)
            changed = [r["upd"][0] + r["upd"][1] for r in recs]
            repairs = [len(r["plan"]["expanded"]) for r in recs[1:]]
            nmax = max(r["n_nodes"] for r in recs)
            print("control", control, "member", k, "first plan", len(recs[0]["plan"]["expanded"]), recs[0]["n_nodes"], "changed", changed,
                  "blocked at tick 3", recs[2]["upd"][0], "repairs", repairs, "largest space", nmax)
            assert sum(changed) > 0 and sum(changed[1:]) > 0 and max(repairs) > 0, (control, k, changed, repairs)
            assert nmax <= CAP[0], (control, k, nmax)
            # (the cap of 5 000 is not met by a first plan, so it is the plan with the cap lifted)
            assert (len(recs[0]["plan"]["expanded"]), recs[0]["n_nodes"]) == FIRST_PLANS[control][k // 2], (control, k)
    for (s, g), n_states in zip(CAPPED_PAIRS, (23642, 24259)):
        for turn in (False, True):
            K = checker(ACC, turn)
            ro = K.lpa_plan(state13(s), state13(g), max_expand=MAX_EXPAND)
            assert ro["status"] == 3 and len(ro["expanded"]) == MAX_EXPAND
            assert K.lpa_state_space()["n_nodes"] == n_states <= CAP[0]
    K = checker(ACC, False)
    ro = K.lpa_plan(state13(BIG_PAIR[0]), state13(BIG_PAIR[1]), max_expand=-1)
    n = K.lpa_state_space()["n_nodes"]
    assert ro["status"] == 0 and (len(ro["expanded"]), n) == (19212, 70098) and CAP[0] < n <= BIG_CAP[0]


def test_library_exports_the_plpa3_fleet_and_capi_binds_it():
    lib = _capi.load()
    for name in FLEET_NAMES:
        assert name in _capi.EXPORTS
        assert getattr(lib, name) is not None
    # null handles are refused without touching a device
    out = C.c_void_p()
    w = np.zeros(4, dtype=np.int32)
    assert lib.mplx_plpa3_fleet_create(None, 4, w.ctypes.data, C.byref(out)) == _capi.ERR_ARG and not out.value
    assert lib.mplx_plpa3_fleet_size(None) == 0 and lib.mplx_plpa3_fleet_last_error(None) == b""
    assert lib.mplx_plpa3_fleet_member(None, 0) is None
    assert lib.mplx_plpa3_fleet_set_capacity(None, 0, 0, 0) == _capi.ERR_ARG and lib.mplx_plpa3_fleet_set_world(None, 0, 0) == _capi.ERR_ARG
    assert lib.mplx_plpa3_fleet_plan(None, None, None, None, 1.0, 0.5, -1.0, -1, 1, None) == _capi.ERR_ARG
    assert lib.mplx_plpa3_fleet_update_nodes(None, None, None) == _capi.ERR_ARG
    assert lib.mplx_plpa3_fleet_sub_state_space(None, None) == _capi.ERR_ARG
    assert lib.mplx_plpa3_fleet_stats(None, None) == _capi.ERR_ARG
    assert lib.mplx_plpa3_fleet_last_kernel_ms(None, None, None) == _capi.ERR_ARG
    lib.mplx_plpa3_fleet_destroy(None)
    assert hasattr(p3, "PolyLpaFleet3D") and hasattr(p3.PolyTeam3D, "lpa_fleet")


def _build_driver(tmp_path):
    exe = str(tmp_path / "plpa3_fleet_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "plpa3_fleet_driver.cpp"), os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def _has_gpu():
    h = C.c_void_p()
    lib = _capi.load()
    if lib.mplx_poly3_create(0, C.byref(h)) == _capi.OK:
        lib.mplx_poly3_destroy(h)
        return True
    return False


def test_plpa3_fleet_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _build_driver(tmp_path)
    if _has_gpu():
        pytest.skip("GPU present")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no HIP device" in out.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU: the sides
class Side:
    """N planners on a PolyTeam3D of their own with the two worlds: as a fleet, or as N single PolyLpa3D handles that get the same
    calls one after the other"""

    def __init__(self, control, world_of, fleet, cap=CAP):
        self.control, self.n = control, len(world_of)
        self.team = p3.PolyTeam3D()
        self.team.configure(control, U27, **KW[control])
        self.team.set_worlds(worlds(0.0))
        self.fleet = self.team.lpa_fleet(world_of) if fleet else None
        self.singles = None if fleet else [p3.PolyLpa3D(self.team, w) for w in world_of]
        for i in range(self.n):
            self.member(i).set_capacity(*cap)

    def member(self, i):
        return self.fleet.member(i) if self.fleet else self.singles[i]

    def set_worlds(self, t):
        self.team.set_worlds(worlds(t))

    def update(self):
        return self.fleet.update_nodes() if self.fleet else [l.update_nodes() for l in self.singles]

    def plan(self, starts, goals, active=None, **kw):
        """-> the n results as dicts (all words zero for an inactive member)"""
        kw.setdefault("max_expand", MAX_EXPAND)
        if self.fleet:
            return [r.as_dict() for r in self.fleet.plan(starts, goals, active, **kw)]
        out = []
        for i, l in enumerate(self.singles):
            if active is not None and not active[i]:
                out.append(_capi.Result().as_dict())
                continue
            l.plan(starts[i], goals[i], **kw)
            out.append(l.result.as_dict())
        return out

    def sub(self, steps):
        if self.fleet:
            self.fleet.sub_state_space(steps)
        else:
            for l, k in zip(self.singles, steps):
                if k >= 0:
                    l.sub_state_space(k)


def snapshot(l):
    """everything a member answers after a plan: expansion order, state space, trajectory"""
    act, ids, st = l.traj()
    return dict(expanded=l.expanded_ids(), space=l.state_space(), act=act, ids=ids, st=st)


def same_snapshots(a, b, where):
    assert np.array_equal(a["expanded"], b["expanded"]), where
    assert a["space"]["initialized"] == b["space"]["initialized"] and a["space"]["n_nodes"] == b["space"]["n_nodes"], where
    for k in KEYS:
        assert np.array_equal(a["space"][k], b["space"][k]), (where, k)
    for k in ("act", "ids", "st"):
        assert np.array_equal(a[k], b[k]), (where, k)


def run_flow(side, members, checkers=None, other=None, recommit=(), ticks=TICKS):
    """The flow on `side` for all members at once.  checkers: one live LpaCheckerWorld per member, driven in step -- every answer is
    compared with it.  other: a second side that gets the same calls -- every answer must be equal on both.  recommit: ticks at which,
    after update_nodes, the worlds are committed AGAIN with the two variants swapped and no second update_nodes.  Returns per tick the
    members' results and, with checkers, the expansions of the checker's plans."""
    n = len(members)
    control = side.control
    starts = [m[1].copy() for m in members]
    goals = [m[2] for m in members]
    t, history, expansions = 0.0, [], []
    for tick in range(ticks):
        for s in (side, other):
            if s is not None:
                s.set_worlds(t)
        if checkers is not None:
            for K, m in zip(checkers, members):
                K.reload(p3.replanner_world3(t, m[0]))
        ud = side.update()
        if checkers is not None:
            for i, K in enumerate(checkers):
                uo = K.lpa_update_nodes()
                assert ud[i] == uo, (tick, i, ud[i][:2], uo[:2])
        if other is not None:
            assert ud == other.update(), tick
        if tick in recommit:
            for s in (side, other):
                if s is not None:
                    s.team.set_worlds(worlds(t)[::-1])
            if checkers is not None:
                for K, m in zip(checkers, members):
                    K.reload(p3.replanner_world3(t, not m[0]))
        res = side.plan(starts, goals)
        if side.fleet:
            st = side.fleet.stats()
            assert st == ([0, 1, n, 0] if tick == 0 else [n, 1, 0, 0]), (tick, st)
        history.append(res)
        if checkers is not None:
            exp = []
            for i, K in enumerate(checkers):
                ro = K.lpa_plan(starts[i], goals[i], max_expand=MAX_EXPAND)
                compare(K, side.member(i), ro, res[i]["status"] == _capi.PLAN_OK, control, (tick, i))
                exp.append(len(ro["expanded"]))
            expansions.append(exp)
        if other is not None:
            ro = other.plan(starts, goals)
            assert res == ro, tick
            for i in range(n):
                same_snapshots(snapshot(side.member(i)), snapshot(other.member(i)), (tick, i))
        trajs = [side.member(i).traj() for i in range(n)]
        assert all(r["status"] == _capi.PLAN_OK and len(tr[0]) > 2 for r, tr in zip(res, trajs)), tick  # (every flow member goes on for five ticks)
        side.sub([1] * n)
        if side.fleet:
            st = side.fleet.stats()
            assert st == [0, 1, n, 0], (tick, st)
        if other is not None:
            other.sub([1] * n)
        for i in range(n):
            sd = side.member(i).state_space()
            if checkers is not None:
                checkers[i].lpa_sub_state_space(1)
                same_spaces(sd, checkers[i].lpa_state_space(), control, (tick, i, "after getSubStateSpace"))
            if other is not None:
                so = other.member(i).state_space()
                for k in KEYS:
                    assert np.array_equal(sd[k], so[k]), (tick, i, k)
            assert len(side.member(i).traj()[0]) == 0  # (the stored trajectory is dropped)
        t += 1.0
        for i in range(n):
            starts[i] = trajs[i][2][1].copy()
            starts[i][12] = t
    return history, expansions


# ---------------------------------------------------------------------------------------------------------------- GPU: the tests
@pytest.mark.gpu
def test_fleet_of_8_acc_members_against_a_checker_each():
    members = acc_members()
    side = Side(ACC, [int(m[0]) for m in members], fleet=True)
    hist, exp = run_flow(side, members, checkers=[checker(ACC, m[0]) for m in members])
    assert all(sum(e[i] for e in exp[1:]) > 0 for i in range(len(members)))  # (every member repaired by expanding states)
    ms = side.fleet.last_kernel_ms()
    print("expansions per tick and member", [[int(r["n_expanded"]) for r in res] for res in hist], "last launch: plan %.3f ms, updateNodes %.3f ms" % ms)


@pytest.mark.gpu
def test_fleet_equals_8_single_handles():
    members = acc_members()
    world_of = [int(m[0]) for m in members]
    run_flow(Side(ACC, world_of, fleet=True), members, other=Side(ACC, world_of, fleet=False))


@pytest.mark.gpu
def test_fleet_of_jrk_members_against_the_checker_and_singles():
    members = jrk_members()
    world_of = [int(m[0]) for m in members]
    run_flow(Side(JRK, world_of, fleet=True), members, checkers=[checker(JRK, m[0]) for m in members], other=Side(JRK, world_of, fleet=False))


@pytest.mark.gpu
def test_mixed_call_repair_fresh_inactive_at_goal_and_capped_in_one_launch():
    """Five members, all in world 1 (turn True).  Call 1 (t = 0) plans 0, 1, 2 from their starts; the world moves to t = 1, update_nodes;
    call 2 has one member of each kind: 0 repairs, 1 plans afresh to another member's goal, 2 is inactive, 3 starts at its goal, 4 is a
    capped pair."""
    acc = acc_members()
    m0, m1, m2 = acc[1], acc[3], acc[7]
    m4 = (True, state13(CAPPED_PAIRS[1][0]), state13(CAPPED_PAIRS[1][1]))  # (the second capped pair: it runs into the cap in the world at t = 1 too)
    assert m0[0] and m1[0] and m2[0]
    goal1b = acc[5][2]
    at_goal = state13((5.0, 5.0, 2.0))
    side = Side(ACC, [1] * 5, fleet=True)
    f = side.fleet
    K = [checker(ACC, True) for _ in range(5)]
    starts = [m0[1], m1[1], m2[1], at_goal, m4[1]]
    goals1 = [m0[2], m1[2], m2[2], at_goal, m4[2]]
    goals2 = [m0[2], goal1b, m2[2], at_goal, m4[2]]
    res = side.plan(starts, goals1, active=[1, 1, 1, 0, 0])
    assert f.stats() == [0, 1, 3, 2]
    first = [K[i].lpa_plan(starts[i], goals1[i], max_expand=MAX_EXPAND) for i in (0, 1, 2)]
    for i in (0, 1, 2):
        compare(K[i], f.member(i), first[i], res[i]["status"] == _capi.PLAN_OK, ACC, ("call 1", i))
    assert res[3] == res[4] == _capi.Result().as_dict() and not f.member(3).initialized() and not f.member(4).initialized()
    side.set_worlds(1.0)
    for k in K:
        k.reload(p3.replanner_world3(1.0, True))
    ud = side.update()
    for i in (0, 1, 2):
        assert ud[i] == K[i].lpa_update_nodes(), i
    assert ud[3] == ud[4] == (0, 0, [])
    before2 = snapshot(f.member(2))
    res = side.plan(starts, goals2, active=[1, 1, 0, 1, 1])
    assert f.stats() == [1, 1, 3, 1]  # repaired: 0; afresh: 1 (new goal), 3 and 4 (they hold no space); skipped: 2
    ro0 = K[0].lpa_plan(starts[0], goals2[0], max_expand=MAX_EXPAND)
    ro1 = K[1].lpa_plan(starts[1], goals2[1], max_expand=MAX_EXPAND)
    compare(K[0], f.member(0), ro0, res[0]["status"] == _capi.PLAN_OK, ACC, "repair")
    compare(K[1], f.member(1), ro1, res[1]["status"] == _capi.PLAN_OK, ACC, "afresh")
    assert ro0["status"] == ro1["status"] == 0 and K[1].lpa_state_space()["states"][0][12] == 0.0
    # the inactive member: result zeroed, space (as update_nodes left it: the checker's) and trajectory untouched
    assert res[2] == _capi.Result().as_dict()
    same_snapshots(before2, snapshot(f.member(2)), "inactive member")
    same_spaces(f.member(2).state_space(), K[2].lpa_state_space(), ACC, "inactive member")
    assert len(before2["act"]) == len(first[2]["actions"]) > 0
    # the member at its goal: status 0, cost 0, nothing expanded, no space -- as the checker
    ro3 = K[3].lpa_plan(starts[3], goals2[3], max_expand=MAX_EXPAND)
    assert res[3]["status"] == ro3["status"] == 0 and res[3]["cost"] == ro3["cost"] == 0.0 and res[3]["n_expanded"] == len(ro3["expanded"]) == 0
    assert not f.member(3).initialized() and not K[3].lpa_state_space()["initialized"]
    # the capped member: status 3 at 5 000 expansions, its space is what the checker keeps of the capped plan
    ro4 = K[4].lpa_plan(starts[4], goals2[4], max_expand=MAX_EXPAND)
    assert res[4]["status"] == ro4["status"] == 3 and res[4]["n_expanded"] == len(ro4["expanded"]) == MAX_EXPAND
    compare(K[4], f.member(4), ro4, False, ACC, "capped")
    assert len(f.member(4).traj()[0]) == 0


@pytest.mark.gpu
def test_one_member_out_of_pool_ends_alone_and_plans_afresh_after_set_capacity():
    """Pools come in chunks of 2^15 states, so the member that runs out is one whose plan needs more: BIG_PAIR planned without the cap
    (70 098 states on the checker) at the capacity of the others; then at BIG_CAP."""
    members = acc_members()[:3] + [(False, state13(BIG_PAIR[0]), state13(BIG_PAIR[1]))]
    big = 3
    K = [checker(ACC, m[0]) for m in members]
    side = Side(ACC, [int(m[0]) for m in members], fleet=True)
    f = side.fleet
    starts, goals = [m[1] for m in members], [m[2] for m in members]
    res = side.plan(starts, goals, max_expand=-1)
    assert f.stats() == [0, 1, 4, 0]
    ro = [K[i].lpa_plan(starts[i], goals[i], max_expand=-1) for i in range(4)]
    assert K[big].lpa_state_space()["n_nodes"] > CAP[0] and all(K[i].lpa_state_space()["n_nodes"] <= CAP[0] for i in range(3))
    for i in range(4):
        if i == big:
            assert res[i]["status"] == _capi.PLAN_POOL_FULL and not f.member(i).initialized() and len(f.member(i).traj()[0]) == 0
        else:
            compare(K[i], f.member(i), ro[i], True, ACC, ("first", i))
    f.member(big).set_capacity(*BIG_CAP)
    res = side.plan(starts, goals, max_expand=-1)
    assert f.stats() == [3, 1, 1, 0]
    compare(K[big], f.member(big), ro[big], True, ACC, "afresh after set_capacity")
    for i in range(3):  # (the others went on with the space they held)
        compare(K[i], f.member(i), K[i].lpa_plan(starts[i], goals[i], max_expand=-1), True, ACC, ("again", i))


@pytest.mark.gpu
def test_trust_entries_with_and_without_update_nodes():
    """Ticks 2 and 3 (0-based) commit the worlds AGAIN after update_nodes -- each member then sees the other variant of the obstacles'
    courses -- without a second update_nodes: the members hold inconsistent states to repair and their entries are out of step with the
    obstacles, so a state that is expanded again must run get_succ again, as the checker's loop always does.  On the other ticks
    update_nodes ran after the last commit and the stored outcomes are read.  Every member expands states on a tick of the first kind
    (asserted on the checker's side)."""
    members = acc_members()
    again = (2, 3)
    hist, exp = run_flow(Side(ACC, [int(m[0]) for m in members], fleet=True), members, checkers=[checker(ACC, m[0]) for m in members], recommit=again)
    for i in range(len(members)):
        assert any(exp[t][i] > 0 for t in again), (i, [e[i] for e in exp])


@pytest.mark.gpu
def test_member_planned_on_its_own_keeps_its_space_and_what_the_fleet_refuses():
    """Two members on the second pair.  Member 0 is planned through its own handle before the fleet's first device call: the fleet's
    first plan repairs it (its space moved into the fleet's arrays) and plans member 1 afresh.  Then what is refused before any launch:
    a world index that is not committed (of an inactive member too), members re-rooted together after plans under different set-ups
    (the message names both), a step beyond the trajectory; and mplx_poly3_config drops the members' spaces."""
    from mpl_ros_amd._capi import MplxError
    members = acc_members()[2:4]
    K = [checker(ACC, m[0]) for m in members]
    side = Side(ACC, [int(m[0]) for m in members], fleet=True)
    f = side.fleet
    starts, goals = [m[1] for m in members], [m[2] for m in members]
    ok = f.member(0).plan(starts[0], goals[0], max_expand=MAX_EXPAND)
    compare(K[0], f.member(0), K[0].lpa_plan(starts[0], goals[0], max_expand=MAX_EXPAND), ok, ACC, "own handle")
    side.set_worlds(1.0)
    for k, m in zip(K, members):
        k.reload(p3.replanner_world3(1.0, m[0]))
    ud = side.update()
    assert ud[0] == K[0].lpa_update_nodes() and ud[0][0] + ud[0][1] > 0 and ud[1] == (0, 0, [])
    res = side.plan(starts, goals)
    assert f.stats() == [1, 1, 1, 0]
    for i in range(2):
        compare(K[i], f.member(i), K[i].lpa_plan(starts[i], goals[i], max_expand=MAX_EXPAND), res[i]["status"] == _capi.PLAN_OK, ACC, ("fleet", i))
    f.set_world(1, 2)
    with pytest.raises(MplxError, match="mplx error %d: member 1: world index" % _capi.ERR_ARG):
        side.plan(starts, goals, active=[1, 0])
    with pytest.raises(MplxError, match="mplx error %d: member 1: world index" % _capi.ERR_ARG):
        f.update_nodes()
    f.set_world(1, 1)
    with pytest.raises(MplxError, match="mplx error %d: member 0: time_step 99 outside" % _capi.ERR_ARG):
        f.sub_state_space([99, -1])
    assert f.member(1).plan(starts[1], goals[1], max_expand=MAX_EXPAND, eps=2.0)
    with pytest.raises(MplxError, match="mplx error %d: member 1 .*another set-up.* member 0" % _capi.ERR_ARG):
        f.sub_state_space([1, 1])
    assert f.member(0).initialized() and len(f.member(0).traj()[0]) > 0  # (nothing was launched, nothing dropped)
    side.team.configure(ACC, U27, **KW[ACC])
    assert f.update_nodes() == [(0, 0, []), (0, 0, [])] and not f.member(0).initialized() and not f.member(1).initialized()


@pytest.mark.gpu
def test_plpa3_fleet_driver_json_equals_the_python_path(tmp_path):
    exe = _build_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == TICKS
    members = acc_members()
    hist, _ = run_flow(Side(ACC, [int(m[0]) for m in members], fleet=True), members)
    for tick, (line, res) in enumerate(zip(lines, hist)):
        assert line["tick"] == tick and len(line["members"]) == len(members)
        for i, (d, r) in enumerate(zip(line["members"], res)):
            cost_bits = int(np.array([r["cost"]]).view(np.uint64)[0])
            assert (d["status"], d["cost_bits"], d["n_expanded"], d["expand_hash"]) == (r["status"], cost_bits, r["n_expanded"], r["expand_hash"]), (tick, i)
