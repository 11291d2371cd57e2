"""Fleets of moving-obstacle LPA* planners (mplx_plpa_fleet_*, poly_map.PolyLpaFleet): N PolyLpa planners on one PolyTeam whose
plan(), update_nodes() and sub_state_space() run for all members in one launch each.  Per member every result must be what the same
sequence of single-handle calls gives, bit for bit -- the standard of tests/test_poly_lpa.py, whose compare / same_spaces are used here.

The members are the fixture tests/golden/plpa_fleet_pairs.json (written by tools/make_plpa_fleet_pairs.py): eight (start -> goal) pairs
on pm.replanner_world at scale 1, each with obstacles that keep their course (turn False, world 0) and that change it (turn True, world
1): 16 ACC members; two pairs whose first plan runs into the cap of 5 000 expansions; the JRK members that complete the flow.  The flow is
the one of tests/test_poly_lpa.py, eight ticks: reload the world at t, updateNodes, plan, getSubStateSpace(1), go on from the second state
of the trajectory with t += 1.

The CPU checker (oracle/refpoly.py: LPA* over the compiled reference environment) keeps ONE state space per process, so a member's
flow is run on it from the first tick to the last and RECORDED (every updateNodes answer, every plan, the state space after every plan
and after every getSubStateSpace); the device sides are compared with the recordings.

CPU: the checker facts the GPU tests rest on; the library exports the fleet; the C++ driver compiles and fails loudly without a GPU.
GPU: fleet against a checker per member, fleet against N single PolyLpa handles, JRK, a mixed call, pool exhaustion, trust_entries, the driver."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd import poly_map as pm
from oracle import refpoly
from tests.test_poly_lpa import COLS, KEYS, KW, compare, same_spaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mpl_ros_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "plpa_fleet_pairs.json")
TICKS = 8
MAX_EXPAND = 5000
CAP = (1 << 15, 1 << 18, 1 << 18)  # states, entries, OPEN-log records per member (the largest space of the fixture holds 8 692 states)
FLEET_NAMES = ["mplx_plpa_fleet_create", "mplx_plpa_fleet_destroy", "mplx_plpa_fleet_last_error", "mplx_plpa_fleet_size", "mplx_plpa_fleet_member",
               "mplx_plpa_fleet_set_capacity", "mplx_plpa_fleet_set_world", "mplx_plpa_fleet_plan", "mplx_plpa_fleet_update_nodes",
               "mplx_plpa_fleet_sub_state_space", "mplx_plpa_fleet_stats", "mplx_plpa_fleet_last_kernel_ms"]

needs_checker = pytest.mark.skipif(not refpoly.available(), reason="oracle/_ref/libpolymap_ref.so not built (make -C oracle ref)")


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def state9(p, t=0.0):
    s = np.zeros(9)
    s[0], s[1], s[8] = p[0], p[1], t
    return s


def acc_members():
    """the 16 ACC members: (turn, start, goal) -- member i lives in world int(turn)"""
    return [(turn, state9(s), state9(g)) for s, g in fixture()["pairs"] for turn in (False, True)]


def capped_members():
    return [(turn, state9(s), state9(g)) for s, g in fixture()["capped_pairs"] for turn in (False, True)]


def jrk_members():
    return [(bool(turn), state9(s), state9(g)) for turn, s, g in fixture()["jrk_members"]]


def worlds(t):
    return [pm.replanner_world(t, False), pm.replanner_world(t, True)]


# ---------------------------------------------------------------------------------------------------------------- the checker
class Recorded:
    """the checker's state space at one moment of a recorded flow, with the face tests.test_poly_lpa.compare asks of a checker"""

    def __init__(self, space):
        self.space = space

    def lpa_state_space(self):
        return self.space


def checker_flow(control, member, ticks=TICKS, skip_update=(), recommit=(), astar=False, max_expand=MAX_EXPAND, keep_spaces=True):
    """The flow of one member on the CPU checker, recorded: per tick dict(t, start, upd, plan, space, sub_space[, astar]).
    skip_update: ticks at which the world moves on but updateNodes is NOT called.  recommit: ticks at which, after updateNodes, the
    world is committed AGAIN -- as the OTHER variant of the obstacles' courses at the same time -- without a second updateNodes.
    astar: also a fresh A* through the same environment."""
    turn, start, goal = member
    R = refpoly.RefWorld(pm.replanner_world(0.0, turn), control, pm.U9, **KW[control])
    A = refpoly.RefWorld(pm.replanner_world(0.0, turn), control, pm.U9, **KW[control]) if astar else None
    R.lpa_reset()
    start, t, recs = start.copy(), 0.0, []
    for tick in range(ticks):
        W = pm.replanner_world(t, turn)
        R.reload(W)
        rec = dict(t=t, start=start.copy(), upd=None, sub_space=None)
        if tick not in skip_update:
            rec["upd"] = R.lpa_update_nodes()
        if tick in recommit:
            R.reload(pm.replanner_world(t, not turn))
        ro = R.lpa_plan(start, goal, max_expand=max_expand)
        rec["plan"] = ro
        ss = R.lpa_state_space()
        rec["space"] = ss if keep_spaces else dict(n_nodes=ss["n_nodes"], initialized=ss["initialized"])
        if astar:
            A.reload(W)
            ra = A.plan(start, goal, max_expand=max_expand)
            rec["astar"] = (ra["status"], ra["cost"], len(ra["expanded"]))
        recs.append(rec)
        if ro["status"] != 0 or len(ro["actions"]) <= 2:
            break
        nid = ro["node_ids"][1]
        R.lpa_sub_state_space(1)
        if keep_spaces:
            rec["sub_space"] = R.lpa_state_space()
        start = ss["states"][nid].copy()
        t += 1.0
        start[8] = t
    R.lpa_reset()
    return recs


_flows = {}


def recorded(control, members, **kw):
    """checker_flow of every member, computed once per (control, member, options)"""
    out = []
    for m in members:
        key = (control, m[0], tuple(m[1]), tuple(m[2]), tuple(sorted(kw.items())))
        if key not in _flows:
            _flows[key] = checker_flow(control, m, **{k: v for k, v in kw.items()})
        out.append(_flows[key])
    return out


def flow_facts(recs):
    """(complete with status 0 on every tick, expansions of the first plan, of ticks 2.., changed entries seen, largest space)"""
    complete = len(recs) == TICKS and all(r["plan"]["status"] == 0 for r in recs)
    changed = sum(r["upd"][0] + r["upd"][1] for r in recs if r["upd"] is not None)
    return complete, len(recs[0]["plan"]["expanded"]), sum(len(r["plan"]["expanded"]) for r in recs[1:]), changed, max(r["space"]["n_nodes"] for r in recs)


# ---------------------------------------------------------------------------------------------------------------- CPU
@needs_checker
def test_checker_facts_of_the_fixture_members():
    """Conditions on the INPUTS of the GPU tests (not measurements), re-derived from the checker: every ACC member completes the
    eight ticks with status 0, its LPA* cost equals a fresh A* through the compiled reference environment at every tick, it sees
    changed entries from updateNodes, at least one of its repairs expands a state, and its space fits CAP; the two capped pairs
    run into the 5 000 cap on the first plan (status 3; the checker keeps what the capped plan built, as a single handle does).  The JRK members of the fixture pass the same conditions."""
    fx = fixture()
    assert len(fx["pairs"]) == 8 and len(fx["capped_pairs"]) == 2 and len(fx["jrk_members"]) <= 4
    firsts, repairs, largest = [], [], 0
    for control, members in ((pm.ACC, acc_members()), (pm.JRK, jrk_members())):
        for m in members:
            recs = checker_flow(control, m, astar=True, keep_spaces=False)
            complete, first, rep, changed, nmax = flow_facts(recs)
            assert complete, (control, m, [r["plan"]["status"] for r in recs])
            for r in recs:
                assert (r["plan"]["status"], r["plan"]["cost"]) == r["astar"][:2], (control, m, r["t"])
            assert changed > 0 and rep > 0, (control, m, changed, rep)
            assert nmax <= CAP[0]
            if control == pm.ACC:
                firsts.append(first); repairs.append(rep); largest = max(largest, nmax)
    print("first plans", firsts, "repairs of ticks 2-8", repairs, "largest space", largest)
    assert len(firsts) == 16
    assert min(firsts) >= 50 and max(firsts) < MAX_EXPAND
    for m in capped_members():
        recs = checker_flow(pm.ACC, m, ticks=1, keep_spaces=False)
        assert recs[0]["plan"]["status"] == 3 and len(recs[0]["plan"]["expanded"]) == MAX_EXPAND


def test_library_exports_the_plpa_fleet_and_capi_binds_it():
    lib = _capi.load()
    for name in FLEET_NAMES:
        assert name in _capi.EXPORTS
        assert getattr(lib, name) is not None
    # null handles are refused without touching a device
    out = C.c_void_p()
    w = np.zeros(4, dtype=np.int32)
    assert lib.mplx_plpa_fleet_create(None, 4, w.ctypes.data, C.byref(out)) == _capi.ERR_ARG and not out.value
    assert lib.mplx_plpa_fleet_size(None) == 0 and lib.mplx_plpa_fleet_last_error(None) == b""
    assert lib.mplx_plpa_fleet_member(None, 0) is None
    assert lib.mplx_plpa_fleet_plan(None, None, None, None, 1.0, 0.5, -1.0, -1, 1, None) == _capi.ERR_ARG
    assert lib.mplx_plpa_fleet_update_nodes(None, None, None) == _capi.ERR_ARG
    assert lib.mplx_plpa_fleet_sub_state_space(None, None) == _capi.ERR_ARG
    assert lib.mplx_plpa_fleet_stats(None, None) == _capi.ERR_ARG
    lib.mplx_plpa_fleet_destroy(None)
    assert hasattr(pm, "PolyLpaFleet") and hasattr(pm.PolyTeam, "lpa_fleet")


def _build_driver(tmp_path):
    exe = str(tmp_path / "plpa_fleet_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "plpa_fleet_driver.cpp"), os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def _has_gpu():
    h = C.c_void_p()
    lib = _capi.load()
    if lib.mplx_poly_create(0, C.byref(h)) == _capi.OK:
        lib.mplx_poly_destroy(h)
        return True
    return False


def test_plpa_fleet_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _build_driver(tmp_path)
    if _has_gpu():
        pytest.skip("GPU present")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no HIP device" in out.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU: the sides
class Side:
    """N planners on a PolyTeam of their own with the two worlds of the fixture: as a fleet, or as N single PolyLpa handles that get
    the same calls one after the other"""

    def __init__(self, control, world_of, fleet, cap=CAP):
        self.control, self.n = control, len(world_of)
        self.team = pm.PolyTeam()
        self.team.configure(control, pm.U9, **KW[control])
        self.team.set_worlds(worlds(0.0))
        self.fleet = self.team.lpa_fleet(world_of) if fleet else None
        self.singles = None if fleet else [pm.PolyLpa(self.team, w) for w in world_of]
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


def run_flow(side, members, recs=None, other=None, skip_update=(), recommit=(), ticks=TICKS):
    """The flow on `side` for all members at once.  recs: the members' recorded checker flows -- every answer is compared with them.
    other: a second side that gets the same calls -- every answer must be equal on both.  Returns per tick the members' results."""
    n = len(members)
    control = side.control
    starts = [m[1].copy() for m in members]
    goals = [m[2] for m in members]
    t, history = 0.0, []
    for tick in range(ticks):
        for s in (side, other):
            if s is not None:
                s.set_worlds(t)
        if tick not in skip_update:
            ud = side.update()
            if recs is not None:
                for i in range(n):
                    assert ud[i] == recs[i][tick]["upd"], (tick, i, ud[i][:2], recs[i][tick]["upd"][:2])
            if other is not None:
                assert ud == other.update(), tick
        if tick in recommit:  # the worlds committed again, with the obstacles' courses swapped, and no updateNodes after it
            for s in (side, other):
                if s is not None:
                    s.team.set_worlds(worlds(t)[::-1])
        res = side.plan(starts, goals)
        if side.fleet:
            st = side.fleet.stats()
            assert st[1] == 1 and st[3] == 0 and (st[0], st[2]) == ((0, n) if tick == 0 else (n, 0)), (tick, st)
        history.append(res)
        if recs is not None:
            for i in range(n):
                rec = recs[i][tick]
                # (on what a state is keyed on: the reference's Waypoint also carries the control input it arrived with as `acc`)
                assert np.array_equal(starts[i][COLS[control]], rec["start"][COLS[control]]), (tick, i)
                l = side.member(i)
                compare(Recorded(rec["space"]), l, rec["plan"], res[i]["status"] == _capi.PLAN_OK, control)
        if other is not None:
            ro = other.plan(starts, goals)
            assert res == ro, tick
            for i in range(n):
                same_snapshots(snapshot(side.member(i)), snapshot(other.member(i)), (tick, i))
        trajs = [side.member(i).traj() for i in range(n)]
        assert all(r["status"] == _capi.PLAN_OK and len(tr[0]) > 2 for r, tr in zip(res, trajs)), tick  # (every fixture member goes on for eight ticks)
        side.sub([1] * n)
        if side.fleet:
            st = side.fleet.stats()
            assert st == [0, 1, n, 0], (tick, st)
        if other is not None:
            other.sub([1] * n)
        for i in range(n):
            sd = side.member(i).state_space()
            if recs is not None:
                same_spaces(sd, recs[i][tick]["sub_space"], control, "after getSubStateSpace")
            if other is not None:
                so = other.member(i).state_space()
                for k in KEYS:
                    assert np.array_equal(sd[k], so[k]), (tick, i, k)
            assert len(side.member(i).traj()[0]) == 0  # (the stored trajectory is dropped)
        t += 1.0
        for i in range(n):
            starts[i] = trajs[i][2][1].copy()
            starts[i][8] = t
    return history


# ---------------------------------------------------------------------------------------------------------------- GPU: the tests
@pytest.mark.gpu
@needs_checker
def test_fleet_of_16_acc_members_against_a_checker_each():
    members = acc_members()
    recs = recorded(pm.ACC, members)
    side = Side(pm.ACC, [int(m[0]) for m in members], fleet=True)
    hist = run_flow(side, members, recs=recs)
    ms = side.fleet.last_kernel_ms()
    print("expansions per tick and member", [[int(r["n_expanded"]) for r in res] for res in hist], "last launch: plan %.3f ms, updateNodes %.3f ms" % ms)


@pytest.mark.gpu
def test_fleet_equals_16_single_handles():
    members = acc_members()
    world_of = [int(m[0]) for m in members]
    run_flow(Side(pm.ACC, world_of, fleet=True), members, other=Side(pm.ACC, world_of, fleet=False))


@pytest.mark.gpu
@needs_checker
def test_fleet_of_jrk_members_against_the_checker_and_singles():
    members = jrk_members()
    if not members:  # (no JRK candidate completed the flow on the checker: tools/make_plpa_fleet_pairs.py records the ones that do)
        return
    recs = recorded(pm.JRK, members)
    world_of = [int(m[0]) for m in members]
    run_flow(Side(pm.JRK, world_of, fleet=True), members, recs=recs, other=Side(pm.JRK, world_of, fleet=False))


def checker_calls(control, turn, calls, max_expand=MAX_EXPAND):
    """a sequence of calls on the checker for ONE member, recorded: calls = [(world time, update?, start, goal)] (start None: no plan)
    -> [(upd, plan, space)]"""
    R = refpoly.RefWorld(pm.replanner_world(0.0, turn), control, pm.U9, **KW[control])
    R.lpa_reset()
    out = []
    for t, update, start, goal in calls:
        R.reload(pm.replanner_world(t, turn))
        upd = R.lpa_update_nodes() if update else None
        ro = R.lpa_plan(start, goal, max_expand=max_expand) if start is not None else None
        out.append((upd, ro, R.lpa_state_space()))
    R.lpa_reset()
    return out


@pytest.mark.gpu
@needs_checker
def test_mixed_call_repair_fresh_inactive_at_goal_and_capped_in_one_launch():
    """Five members, all in world 1 (turn True).  Call 1 (t = 0) plans 0, 1, 2 from their starts; the world moves to t = 1, update_nodes;
    call 2 has one member of each kind: 0 repairs, 1 plans afresh to a new goal, 2 is inactive, 3 starts at its goal, 4 is a capped pair."""
    acc, cap = acc_members(), capped_members()
    m0, m1, m2, m4 = acc[1], acc[5], acc[9], cap[3]  # (the second capped pair: it runs into the cap in the world at t = 1 too)
    assert m0[0] and m1[0] and m2[0] and m4[0]
    goal1b = acc[13][2]
    at_goal = state9((5.0, 5.0))
    side = Side(pm.ACC, [1] * 5, fleet=True)
    f = side.fleet
    starts = [m0[1], m1[1], m2[1], at_goal, m4[1]]
    goals1 = [m0[2], m1[2], m2[2], at_goal, m4[2]]
    goals2 = [m0[2], goal1b, m2[2], at_goal, m4[2]]
    want = {0: checker_calls(pm.ACC, True, [(0.0, False, m0[1], m0[2]), (1.0, True, m0[1], m0[2])]),
            1: checker_calls(pm.ACC, True, [(0.0, False, m1[1], m1[2]), (1.0, True, m1[1], goal1b)]),
            2: checker_calls(pm.ACC, True, [(0.0, False, m2[1], m2[2]), (1.0, True, None, None)]),
            3: checker_calls(pm.ACC, True, [(1.0, False, at_goal, at_goal)]),
            4: checker_calls(pm.ACC, True, [(1.0, False, m4[1], m4[2])])}
    res = side.plan(starts, goals1, active=[1, 1, 1, 0, 0])
    assert f.stats() == [0, 1, 3, 2]
    for i in (0, 1, 2):
        compare(Recorded(want[i][0][2]), f.member(i), want[i][0][1], res[i]["status"] == _capi.PLAN_OK, pm.ACC)
    assert res[3] == res[4] == _capi.Result().as_dict() and not f.member(3).initialized() and not f.member(4).initialized()
    side.set_worlds(1.0)
    ud = side.update()
    assert ud[0] == want[0][1][0] and ud[1] == want[1][1][0] and ud[2] == want[2][1][0] and ud[3] == ud[4] == (0, 0, [])
    before2 = snapshot(f.member(2))
    res = side.plan(starts, goals2, active=[1, 1, 0, 1, 1])
    assert f.stats() == [1, 1, 3, 1]  # repaired: 0; afresh: 1 (new goal), 3 and 4 (they hold no space); skipped: 2
    compare(Recorded(want[0][1][2]), f.member(0), want[0][1][1], res[0]["status"] == _capi.PLAN_OK, pm.ACC)
    compare(Recorded(want[1][1][2]), f.member(1), want[1][1][1], res[1]["status"] == _capi.PLAN_OK, pm.ACC)
    assert res[0]["status"] == res[1]["status"] == _capi.PLAN_OK
    # the inactive member: result zeroed, space (as update_nodes left it: the checker's) and trajectory untouched
    assert res[2] == _capi.Result().as_dict()
    same_snapshots(before2, snapshot(f.member(2)), "inactive member")
    same_spaces(f.member(2).state_space(), want[2][1][2], pm.ACC, "inactive member")
    assert len(before2["act"]) == len(want[2][0][1]["actions"]) > 0
    # the member at its goal: status 0, cost 0, nothing expanded, no space -- as the checker
    ro3 = want[3][0][1]
    assert res[3]["status"] == ro3["status"] == 0 and res[3]["cost"] == ro3["cost"] == 0.0 and res[3]["n_expanded"] == len(ro3["expanded"]) == 0
    assert not f.member(3).initialized() and not want[3][0][2]["initialized"]
    # the capped member: status as the checker's, no space
    ro4 = want[4][0][1]
    assert res[4]["status"] == ro4["status"] == 3 and res[4]["n_expanded"] == len(ro4["expanded"]) == MAX_EXPAND
    compare(Recorded(want[4][0][2]), f.member(4), ro4, False, pm.ACC)  # (the space of a capped plan is what the checker keeps of it)
    assert len(f.member(4).traj()[0]) == 0


@pytest.mark.gpu
@needs_checker
def test_one_member_out_of_pool_ends_alone_and_plans_afresh_after_set_capacity():
    """Pools come in chunks of 2^15 states, so the member that runs out is one whose first plan needs more: the second capped pair
    planned WITHOUT the cap (266 710 states on the checker) at the capacity of the others; then at 2^19 states / 2^21 entries."""
    members = acc_members()[:3] + [capped_members()[2]]
    big = 3
    want = [checker_calls(pm.ACC, m[0], [(0.0, False, m[1], m[2])] * (1 if i == big else 2), max_expand=-1) for i, m in enumerate(members)]
    assert want[big][0][2]["n_nodes"] > CAP[0] and all(want[i][0][2]["n_nodes"] <= CAP[0] for i in range(3))
    side = Side(pm.ACC, [int(m[0]) for m in members], fleet=True)
    f = side.fleet
    starts, goals = [m[1] for m in members], [m[2] for m in members]
    res = side.plan(starts, goals, max_expand=-1)
    assert f.stats() == [0, 1, 4, 0]
    for i in range(4):
        if i == big:
            assert res[i]["status"] == _capi.PLAN_POOL_FULL and not f.member(i).initialized() and len(f.member(i).traj()[0]) == 0
        else:
            compare(Recorded(want[i][0][2]), f.member(i), want[i][0][1], True, pm.ACC)
    f.member(big).set_capacity(1 << 19, 1 << 21, 1 << 21)
    res = side.plan(starts, goals, max_expand=-1)
    assert f.stats() == [3, 1, 1, 0]
    compare(Recorded(want[big][0][2]), f.member(big), want[big][0][1], True, pm.ACC)
    for i in range(3):  # (the others went on with the space they held)
        compare(Recorded(want[i][1][2]), f.member(i), want[i][1][1], True, pm.ACC)


@pytest.mark.gpu
@needs_checker
def test_trust_entries_with_and_without_update_nodes():
    """Ticks 3, 4 and 6 commit the worlds AGAIN after update_nodes -- each member then sees the other variant of the obstacles' courses --
    without a second update_nodes: the members hold inconsistent states to repair and their entries are out of step with the obstacles,
    so a state that is expanded again must run get_succ again, as the checker's loop always does.  On the other ticks update_nodes ran
    after the last commit and the stored outcomes are read.  Every member expands states on a tick of the first kind here (checked
    on the recordings); on ticks of the second kind every member does in test_fleet_of_16_acc_members_against_a_checker_each, whose
    ticks are all of that kind."""
    members = acc_members()
    again = (2, 3, 5)
    recs = recorded(pm.ACC, members, recommit=again)
    for r in recs:
        assert any(len(r[t]["plan"]["expanded"]) > 0 for t in again)
    assert any(len(r[t]["plan"]["expanded"]) > 0 for r in recs for t in range(1, TICKS) if t not in again)
    run_flow(Side(pm.ACC, [int(m[0]) for m in members], fleet=True), members, recs=recs, recommit=again)


@pytest.mark.gpu
def test_plpa_fleet_driver_json_equals_the_python_path(tmp_path):
    exe = _build_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == TICKS
    members = acc_members()
    hist = run_flow(Side(pm.ACC, [int(m[0]) for m in members], fleet=True), members)
    for tick, (line, res) in enumerate(zip(lines, hist)):
        assert line["tick"] == tick and len(line["members"]) == 16
        for i, (d, r) in enumerate(zip(line["members"], res)):
            cost_bits = int(np.array([r["cost"]]).view(np.uint64)[0])
            assert (d["status"], d["cost_bits"], d["n_expanded"], d["expand_hash"]) == (r["status"], cost_bits, r["n_expanded"], r["expand_hash"]), (tick, i)
