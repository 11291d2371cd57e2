"""LPA* fleets (mplx_lpa_fleet_*, planner.LpaFleet): N LPA* planners on one MapUtil whose plan() and map updates run for all
members in one launch.  Per member every result must be what the same sequence of single-planner calls gives, bit for bit -- the
standard of tests/test_lpa.py, whose Scenario / compare_lpa / box_cells are used here.

Scenarios (the pairs are the fixture tests/golden/lpa_fleet_pairs.json, written by tools/make_lpa_fleet_pairs.py):
  F2  2-D lattice, simple_map.npz, set-up KW, 16 members; a wall (9.05, 5.05) -> (9.05, 13.05) is added, later cleared.
  F3  27 inputs, skir_map.npz, KW3, 8 members; the union of a 5^3 box on the middle of every member's first path.
  FJ  125 inputs (JERK), the map / set-up / capacities of test_hip_lpastar_imports_a_jerk_lattice_plan_bit_exact..., 4 members;
      the union of a 3^3 box on the middle of every member's first path.

CPU: the inputs are what the GPU tests need them to be (every member keeps a path, LPA* == fresh A* on the checker, most
repairs expand a state); the library exports the fleet; the C++ driver compiles and fails loudly without a GPU.
GPU: fleet against a CPU checker LPA* per member, fleet against N single planners, mixed calls, pool exhaustion, the driver."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mpl_ros_amd import _capi, mapgen
from oracle import orc
from tests import util
from tests.test_lpa import KW, KW3, Scenario, box_cells, compare_lpa, scenario_3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mpl_ros_amd", "csrc")
WALL = ((9.05, 5.05, 0.025), (9.05, 13.05, 0.025))
RAY2 = ((8.05, 3.05, 0.025), (10.05, 15.05, 0.025))
FLEET_NAMES = ["mplx_lpa_fleet_create", "mplx_lpa_fleet_destroy", "mplx_lpa_fleet_last_error", "mplx_lpa_fleet_size", "mplx_lpa_fleet_member",
               "mplx_lpa_fleet_set_capacity", "mplx_lpa_fleet_plan", "mplx_lpa_fleet_update_blocked", "mplx_lpa_fleet_update_cleared",
               "mplx_lpa_fleet_sub_state_space", "mplx_lpa_fleet_stats", "mplx_lpa_fleet_last_kernel_ms"]


def pairs(name):
    with open(os.path.join(ROOT, "tests", "golden", "lpa_fleet_pairs.json")) as f:
        return [(tuple(s), tuple(g)) for s, g in json.load(f)[name]]


# ---------------------------------------------------------------------------------------------------------------- the scenarios
class Case:
    """One scenario: the map, the lattice, the pairs; N CPU-checker LPA* planners (and, for the CPU test, N fresh A*)."""

    def __init__(self, name):
        self.name = name
        if name == "F2":
            self.sc = Scenario()
            self.grid, self.origin, self.res, self.U, self.kw, self.control = self.sc.grid, self.sc.origin, self.sc.res, self.sc.U, KW, orc.ACC
            self.pairs = pairs("F2")
            self.cap = (1 << 17, 1 << 19, 1 << 19)
        elif name == "F3":
            self.grid, self.origin, self.res, _, _, _ = scenario_3d("skir")
            self.U, self.kw, self.control = mapgen.control_lattice(1.0, 1, True), KW3, orc.ACC
            self.pairs = pairs("F3")
            self.cap = (1 << 19, 1 << 22, 1 << 21)
        else:
            self.grid, self.origin, self.res = util.small_map(64, seed=21, occupancy=0.06)
            self.U, self.control = mapgen.control_lattice(1.0, 2, True), orc.JRK
            self.kw = dict(v_max=2.0, a_max=1.0, j_max=1.0, tol_pos=0.5, max_expand=4000)
            a, b = 0.55, 5.55
            self.pairs = [((a, a, a), (b, b, b)), ((b, b, b), (a, a, a)), ((a, b, a), (b, a, b)), ((b, a, a), (a, b, b))]
            self.cap = (1 << 19, 1 << 22, 1 << 21)
        self.n = len(self.pairs)
        self.grid0 = self.grid.copy()
        self.scratch = util.make_oracle(self.grid, self.origin, self.res, self.control, self.U, **self.kw)
        self.L = [self.oracle(True) for _ in range(self.n)]

    def oracle(self, lpa):
        P = util.make_oracle(self.grid, self.origin, self.res, self.control, self.U, **self.kw)
        P.set_lpastar(lpa)
        return P

    def o_wp(self, p, vel=(0, 0, 0), acc=(0, 0, 0)):
        return orc.waypoint(tuple(p), vel=tuple(vel), acc=tuple(acc), control=self.control)

    def g_wp(self, p, vel=(0, 0, 0), acc=(0, 0, 0)):
        return util.gpu_wp(tuple(p), vel=tuple(vel), acc=tuple(acc), control=self.control)

    def starts(self, g=False):
        return [(self.g_wp if g else self.o_wp)(s) for s, _ in self.pairs]

    def goals(self, g=False):
        return [(self.g_wp if g else self.o_wp)(t) for _, t in self.pairs]

    # ---- the edit of the scenario, from the checkers' first trajectories; the map of every checker follows
    def block_cells(self):
        if self.name == "F2":
            return self.sc.add(*WALL)  # (edits self.grid: whole columns)
        half = 2 if self.name == "F3" else 1
        cells = set()
        for L in self.L:
            tr = L.traj()
            cells |= set(box_cells(self.scratch, tuple(tr["wps"][tr["n"] // 2].pos), half))
        cells = sorted(cells)
        for x, y, z in cells:
            self.grid[z, y, x] = 100
        return cells

    def unblock(self, cells):
        if self.name == "F2":
            self.sc.clear_cells(cells)
        else:
            for x, y, z in cells:
                self.grid[z, y, x] = 0

    def set_maps(self, planners, mu=None):
        self.scratch.set_map(self.grid, self.origin, self.res)
        for P in planners:
            P.set_map(self.grid, self.origin, self.res)
        if mu is not None:
            dz, dy, dx = self.grid.shape
            mu.setMap(self.origin, (dx, dy, dz), self.grid.ravel(), self.res)

    def o_plan(self, starts=None, members=None):
        """plan() of the checkers' LPA* planners (all, or `members`); the statuses"""
        starts = starts or self.starts()
        out = {}
        for i in (range(self.n) if members is None else members):
            self.L[i].reset_counters()
            out[i] = self.L[i].plan(starts[i], self.goals()[i])
        return out

    # ---- the device side
    def gpu(self):
        mu, a = util.make_gpu(self.grid, self.origin, self.res, self.U, **self.kw)
        return mu, a

    def setup(self, pl):
        kw = self.kw
        pl.setVmax(kw["v_max"]); pl.setAmax(kw["a_max"]); pl.setJmax(kw.get("j_max", -1.0)); pl.setDt(1.0); pl.setU(self.U)
        pl.setTol(kw["tol_pos"], kw.get("tol_vel", -1.0), kw.get("tol_acc", -1.0)); pl.setMaxNum(kw.get("max_expand", -1))
        pl.setCapacity(1, *self.cap)
        return pl

    def fleet(self, mu):
        from mpl_ros_amd.planner import LpaFleet
        return self.setup(LpaFleet(mu, self.n))

    def singles(self, mu):
        from mpl_ros_amd.planner import VoxelMapPlanner
        out = []
        for _ in range(self.n):
            pl = VoxelMapPlanner(False)
            pl.setMapUtil(mu)
            self.setup(pl)
            pl.setLPAstar(True)
            out.append(pl)
        return out


def compare_member(case, L, view, r, st_o):
    """fleet member `view` (result r) against its CPU checker LPA* L: compare_lpa; JERK states for FJ"""
    if case.control == orc.ACC:
        compare_lpa(L, view, r, st_o)
        return
    assert r.status == st_o
    ids = L.expanded()[0]
    assert r.n_expanded == L.lpa_iterations() == len(ids) and r.expand_hash == util.expand_hash(ids)
    ss = view.lpaStateSpace()
    n = L.num_nodes()
    assert ss["n_nodes"] == n == r.n_nodes
    g = np.array([L.node(i)[1] for i in range(n)]); h = np.array([L.node(i)[2] for i in range(n)])
    closed = np.array([L.node(i)[3] for i in range(n)], dtype=np.int32)
    rhs = np.array([L.node_rhs(i) for i in range(n)]); opened = np.array([L.node_opened(i) for i in range(n)], dtype=np.int32)
    assert np.array_equal(ss["g"], g) and np.array_equal(ss["rhs"], rhs) and np.array_equal(ss["h"], h)
    assert np.array_equal(ss["closed"], closed) and np.array_equal(ss["opened"], opened)
    co, po, ao = L.edges()
    assert np.array_equal(ss["child"], co) and np.array_equal(ss["parent"], po) and np.array_equal(ss["action"], ao)
    assert np.array_equal(ss["blocked"], L.edges_blocked())
    assert r.n_closed == L.num_closed()
    if st_o == orc.OK:
        assert r.cost == L.traj_cost
        to, tg = L.traj(), view.getTraj()
        assert np.array_equal(tg.actions, to["actions"]) and np.array_equal(tg.node_ids, to["node_ids"])
        for wg, wo in zip(tg.getWaypoints(), to["wps"]):
            assert np.array_equal(wg.state(), orc.wp_state(wo, orc.JRK))


RECORD = ("status", "cost", "n_expanded", "expand_hash", "n_nodes", "n_edges", "n_closed", "traj_len")


def same_planner_state(a, ra, b, rb):
    """two device planners (views) after the same calls: result record, state space, trajectory"""
    for k in RECORD:
        assert getattr(ra, k) == getattr(rb, k), k
    assert a.initialized() == b.initialized()
    if a.initialized():
        sa, sb = a.lpaStateSpace(), b.lpaStateSpace()
        assert sa["n_nodes"] == sb["n_nodes"] and sa["n_edges"] == sb["n_edges"] and sa["n_blocked_log"] == sb["n_blocked_log"]
        for k in ("pos", "g", "rhs", "h", "closed", "opened", "built", "child", "parent", "action", "blocked"):
            assert np.array_equal(sa[k], sb[k]), k
    ta, tb = a.getTraj(), b.getTraj()
    assert np.array_equal(ta.actions, tb.actions)
    assert len(ta.getWaypoints()) == len(tb.getWaypoints())
    for wa, wb in zip(ta.getWaypoints(), tb.getWaypoints()):
        assert np.array_equal(wa.state(), wb.state())
    if len(ta.actions):
        assert np.array_equal(ta.node_ids, tb.node_ids)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name,min_repairs", [("F2", 12), ("F3", 8), ("FJ", 3)])
def test_checker_lpastar_equals_fresh_astar_for_every_member(name, min_repairs):
    """Conditions on the INPUTS of the GPU tests (not measurements): after every step the CPU checker's LPA* equals its fresh A*
    for every member and every member keeps a path; after the blocking edit at least 12 of 16 (F2), 8 of 8 (F3), 3 of 4 (FJ, the
    union of the four boxes) repairs expand a state; after the clearing every member is back at its first cost."""
    case = Case(name)
    A = [case.oracle(False) for _ in range(case.n)]

    def both():
        st = case.o_plan()
        rows = []
        for i in range(case.n):
            sa = A[i].plan(case.starts()[i], case.goals()[i])
            assert sa == st[i] == orc.OK, (name, i, sa, st[i])
            assert A[i].traj_cost == case.L[i].traj_cost, (name, i)
            rows.append((case.L[i].lpa_iterations(), case.L[i].traj_cost))
        return rows

    r0 = both()
    assert all(it > 0 for it, _ in r0)
    cells = case.block_cells()
    if name == "F2":
        assert len(cells) == 1975
    case.set_maps(A + case.L)
    changed = [L.update_blocked(cells) for L in case.L]
    r1 = both()
    repaired = sum(1 for it, _ in r1 if it > 0)
    print(name, "cells", len(cells), "first", [it for it, _ in r0], "entries", changed, "repairs", [it for it, _ in r1])
    assert repaired >= min_repairs
    case.unblock(cells)
    case.set_maps(A + case.L)
    for L in case.L:
        L.update_cleared(cells)
    r2 = both()
    assert [c for _, c in r2] == [c for _, c in r0]


def test_second_ray_of_f2_touches_every_member():
    """the second edit of F2, (8.05, 3.05) -> (10.05, 15.05): every member's state space holds entries it blocks"""
    case = Case("F2")
    assert all(s == orc.OK for s in case.o_plan().values())
    cells = case.sc.add(*RAY2)
    case.set_maps(case.L)
    assert all(L.update_blocked(cells) > 0 for L in case.L)


def test_library_exports_the_fleet_and_capi_binds_it():
    lib = _capi.load()
    for name in FLEET_NAMES:
        assert name in _capi.EXPORTS
        assert getattr(lib, name) is not None
    # null handles are refused without touching a device
    out = C.c_void_p()
    assert lib.mplx_lpa_fleet_create(None, 4, C.byref(out)) == _capi.ERR_ARG and not out.value
    assert lib.mplx_lpa_fleet_size(None) == 0 and lib.mplx_lpa_fleet_last_error(None) == b""
    assert lib.mplx_lpa_fleet_member(None, 0) is None
    assert lib.mplx_lpa_fleet_plan(None, None, None, None, None) == _capi.ERR_ARG
    assert lib.mplx_lpa_fleet_update_blocked(None, 0, None, None) == _capi.ERR_ARG
    assert lib.mplx_lpa_fleet_stats(None, None) == _capi.ERR_ARG
    lib.mplx_lpa_fleet_destroy(None)
    from mpl_ros_amd.planner import LpaFleet  # noqa: F401


def _build_driver(tmp_path):
    exe = str(tmp_path / "lpa_fleet_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "lpa_fleet_driver.cpp"), os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def _has_gpu():
    h = C.c_void_p()
    lib = _capi.load()
    if lib.mplx_ctx_create(0, C.byref(h)) == _capi.OK:
        lib.mplx_ctx_destroy(h)
        return True
    return False


def test_fleet_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _build_driver(tmp_path)
    if _has_gpu():
        pytest.skip("GPU present")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no HIP device" in out.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU
def check_fleet(case, fleet, res, st_o, members=None):
    for i in (range(case.n) if members is None else members):
        assert (res[i].status == _capi.PLAN_OK) == (st_o[i] == orc.OK)
        compare_member(case, case.L[i], fleet.member(i), res[i], st_o[i])


def replay(case, sides, mu, check, sub_state_space=True):
    """The scenario on every side of `sides` (objects with plan / blocked / cleared / sub): first plan, the blocking edit,
    plan, the clearing, plan, [getSubStateSpace(1) of every member, plan from every member's second waypoint].
    check(label, per-side plan results or None, per-side update counts or None) after every step."""
    def plan_all(label, starts_o=None, starts_g=None):
        check(label, [s.plan(starts_o, starts_g) for s in sides], None)

    plan_all("first")
    cells = case.block_cells()
    case.set_maps(case.L, mu)
    check("block", None, [s.blocked(cells) for s in sides])
    plan_all("blocked")
    case.unblock(cells)
    case.set_maps(case.L, mu)
    check("clear", None, [s.cleared(cells) for s in sides])
    plan_all("cleared")
    if sub_state_space:
        w1 = [L.traj()["wps"][1] for L in case.L]
        for s in sides:
            s.sub(1)
        plan_all("moved on", [case.o_wp(w.pos, w.vel, w.acc) for w in w1], [case.g_wp(w.pos, w.vel, w.acc) for w in w1])


class CheckerSide:
    def __init__(self, case):
        self.case = case

    def plan(self, starts_o, starts_g):
        return self.case.o_plan(starts_o)

    def blocked(self, cells):
        return [L.update_blocked(cells) for L in self.case.L]

    def cleared(self, cells):
        return [L.update_cleared(cells) for L in self.case.L]

    def sub(self, k):
        for L in self.case.L:
            L.sub_state_space(k)


class FleetSide:
    def __init__(self, case, fleet):
        self.case, self.fleet, self.stats = case, fleet, []

    def plan(self, starts_o, starts_g):
        res = self.fleet.plan(starts_g or self.case.starts(True), self.case.goals(True))
        self.stats.append(self.fleet.stats())
        return res

    def blocked(self, cells):
        return self.fleet.updateBlockedNodes(cells)

    def cleared(self, cells):
        return self.fleet.updateClearedNodes(cells)

    def sub(self, k):
        self.fleet.getSubStateSpace([k] * self.case.n)

    def view(self, i):
        return self.fleet.member(i)


class SinglesSide:
    def __init__(self, case, planners):
        self.case, self.pl = case, planners

    def plan(self, starts_o, starts_g):
        starts_g = starts_g or self.case.starts(True)
        out = []
        for i, pl in enumerate(self.pl):
            pl.plan(starts_g[i], self.case.goals(True)[i])
            out.append(pl.getResult())
        return out

    def blocked(self, cells):
        return [pl.updateBlockedNodes(cells) for pl in self.pl]

    def cleared(self, cells):
        return [pl.updateClearedNodes(cells) for pl in self.pl]

    def sub(self, k):
        for pl in self.pl:
            pl.getSubStateSpace(k)

    def view(self, i):
        return self.pl[i]


def fleet_against_checker(name, sub_state_space, fresh_astar=False):
    case = Case(name)
    mu, a = case.gpu()
    fleet = case.fleet(mu)
    if fresh_astar:
        a.setCapacity(case.n, 1 << 20, 1 << 22, 1 << 21)  # (a batch's pools are shared by its queries, one slot each)
    fs = FleetSide(case, fleet)
    seen = []

    def check(label, res, counts):
        seen.append(label)
        if counts is not None:
            print(name, label, counts[1])
            assert counts[1] == counts[0]  # per member, the checker's
            return
        st_o, rg = res
        print(name, label, "expanded", [int(r.n_expanded) for r in rg], "stats", fs.stats[-1], "ms", fleet.lastKernelMs())
        check_fleet(case, fleet, rg, st_o)
        assert all(st_o[i] == orc.OK for i in range(case.n))
        assert fs.stats[-1] == ([0, 0, case.n, 0] if label == "first" else [case.n, 1, 0, 0])
        if fresh_astar:  # LPA* cost == a fresh device A* of the same queries
            starts = [case.g_wp(w.pos, w.vel, w.acc) for w in (fleet.getTraj(i).getWaypoints()[0] for i in range(case.n))]
            ra = a.planBatch(starts, case.goals(True))
            assert [r.cost for r in ra] == [r.cost for r in rg]

    replay(case, [CheckerSide(case), fs], mu, check, sub_state_space)
    assert seen == ["first", "block", "blocked", "clear", "cleared"] + (["moved on"] if sub_state_space else [])
    assert fleet.initialized() == [True] * case.n


@pytest.mark.gpu
def test_fleet_replays_f2_against_a_checker_per_member():
    """F2: fleet.plan -> wall -> updateBlockedNodes -> plan -> clear_cells -> updateClearedNodes -> plan -> getSubStateSpace(1) of
    every member -> plan from each member's second waypoint; after every step compare_lpa of each of the 16 members against a CPU
    checker LPA* of its own, update counts per member, stats() [0, 0, 16, 0] after the first plan and [16, 1, 0, 0] after every
    later one."""
    fleet_against_checker("F2", True)


@pytest.mark.gpu
def test_fleet_equals_sixteen_single_planners_on_f2():
    """the same sequence on 16 separate VoxelMapPlanner(setLPAstar(True)) on the same MapUtil: per member the result record, the
    state space and the trajectory are equal after every step"""
    case = Case("F2")
    mu, _ = case.gpu()
    fs, ss = FleetSide(case, case.fleet(mu)), SinglesSide(case, case.singles(mu))

    def check(label, res, counts):
        if counts is not None:
            assert counts[1] == counts[2] == counts[0]
            return
        _, rf, rs = res
        for i in range(case.n):
            same_planner_state(fs.view(i), rf[i], ss.view(i), rs[i])

    replay(case, [CheckerSide(case), fs, ss], mu, check, True)


@pytest.mark.gpu
def test_fleet_replays_f3_against_the_checker_and_a_fresh_device_astar():
    """F3 (27 inputs, 8 members): every member against the checker after every step; cost == planBatch of the 8 queries"""
    fleet_against_checker("F3", False, fresh_astar=True)


@pytest.mark.gpu
def test_fleet_jerk_lattice_equals_singles_and_the_checker():
    """FJ (125 inputs: the 128-lane builds): fleet equals singles and the checker after the block and after the clear"""
    case = Case("FJ")
    mu, _ = case.gpu()
    fleet = case.fleet(mu)
    fs, ss = FleetSide(case, fleet), SinglesSide(case, case.singles(mu))

    def check(label, res, counts):
        if counts is not None:
            assert counts[1] == counts[2] == counts[0]
            return
        st_o, rf, rs = res
        print("FJ", label, "expanded", [int(r.n_expanded) for r in rf], "stats", fs.stats[-1])
        check_fleet(case, fleet, rf, st_o)
        for i in range(case.n):
            same_planner_state(fs.view(i), rf[i], ss.view(i), rs[i])
        assert fs.stats[-1] == ([0, 0, 4, 0] if label == "first" else [4, 1, 0, 0])

    replay(case, [CheckerSide(case), fs, ss], mu, check, False)


@pytest.mark.gpu
def test_mixed_fleet_call_on_f2():
    """One plan() with members that repair, one whose goal changed (fresh), one inactive (its space and stored trajectory
    untouched), one whose start cell was blocked by the edit (status 2, from the fleet launch) and one already at its goal (status
    0, cost 0).  The member at its goal never holds a state space -- a plan that does not search leaves none -- so mplx_lpa_plan's
    rule plans it afresh like the member whose goal changed: stats() is [13, 1, 2, 1].  Every member equals a single planner given
    the same calls; the repairing members equal their checkers."""
    case = Case("F2")
    mu, _ = case.gpu()
    fleet, singles = case.fleet(mu), case.singles(mu)
    GOAL_CHANGED, INACTIVE, OCCUPIED, AT_GOAL = 2, 5, 7, 11
    starts, goals = case.starts(True), case.goals(True)
    goals[AT_GOAL] = case.g_wp(case.pairs[AT_GOAL][0])
    special = (GOAL_CHANGED, INACTIVE, OCCUPIED, AT_GOAL)
    repairers = [i for i in range(case.n) if i not in special]

    def singles_plan(active):
        out = []
        for i, pl in enumerate(singles):
            if active[i]:
                pl.plan(starts[i], goals[i])
            out.append(pl.getResult())
        return out

    everyone = [1] * case.n
    r0 = fleet.plan(starts, goals)
    s0 = singles_plan(everyone)
    st0 = case.o_plan(members=repairers)
    assert fleet.stats() == [0, 0, 16, 0]
    assert r0[AT_GOAL].status == 0 and r0[AT_GOAL].cost == 0.0 and not fleet.initialized(AT_GOAL)
    for i in range(case.n):
        same_planner_state(fleet.member(i), r0[i], singles[i], s0[i])
    check_fleet(case, fleet, r0, st0, repairers)
    kept = fleet.lpaStateSpace(INACTIVE)
    kept_traj = fleet.getTraj(INACTIVE)
    # the wall of F2 and the start cell of one member
    cells = case.sc.add(*WALL)
    occ = tuple(int(v) for v in case.scratch.float_to_int(case.pairs[OCCUPIED][0]))
    assert case.scratch.cell_state(occ) == 0
    cells = cells + [occ]
    case.sc.grid[:, occ[1], occ[0]] = 100
    case.set_maps(case.L, mu)
    cf = fleet.updateBlockedNodes(cells)
    cs = [pl.updateBlockedNodes(cells) for pl in singles]
    assert cf == cs and cf[AT_GOAL] == 0
    for i in repairers:
        assert cf[i] == case.L[i].update_blocked(cells)
    goals[GOAL_CHANGED] = case.g_wp(case.pairs[(GOAL_CHANGED + 1) % case.n][1])
    active = [0 if i == INACTIVE else 1 for i in range(case.n)]
    r1 = fleet.plan(starts, goals, active)
    s1 = singles_plan(active)
    assert fleet.stats() == [13, 1, 2, 1]
    assert r1[INACTIVE] is None
    assert r1[OCCUPIED].status == 2
    assert r1[AT_GOAL].status == 0 and r1[AT_GOAL].cost == 0.0 and not fleet.initialized(AT_GOAL)
    assert r1[GOAL_CHANGED].status == 0 and fleet.initialized(GOAL_CHANGED)
    for i in range(case.n):
        if i != INACTIVE:
            same_planner_state(fleet.member(i), r1[i], singles[i], s1[i])
    st1 = case.o_plan(members=repairers)
    check_fleet(case, fleet, r1, st1, repairers)
    assert sum(1 for i in repairers if r1[i].n_expanded > 0) >= 8
    # the inactive member: no search ran on it (its entries carry the blocked bits and its states the rhs of the update, like the
    # single planner's that was not asked to plan)
    now = fleet.lpaStateSpace(INACTIVE)
    for k in ("g", "h", "child", "parent", "action"):
        assert np.array_equal(kept[k], now[k]), k
    assert np.array_equal(kept_traj.actions, fleet.getTraj(INACTIVE).actions)
    same_planner_state(fleet.member(INACTIVE), r0[INACTIVE], singles[INACTIVE], s0[INACTIVE])


@pytest.mark.gpu
def test_one_member_out_of_pool_ends_alone_and_plans_afresh_after_set_capacity():
    """F3: the member with the largest first search (16 155 expansions on the checker) gets pools of one chunk each: it ends
    MPLX_PLAN_POOL_FULL and is not initialized, the others are unaffected; with its capacity restored it plans afresh in the next
    fleet call."""
    case = Case("F3")
    mu, _ = case.gpu()
    fleet = case.fleet(mu)
    st = case.o_plan()
    small = int(np.argmax([L.lpa_iterations() for L in case.L]))
    assert case.L[small].lpa_iterations() > 10000 and len(case.L[small].edges()[0]) > 1 << 16  # (more entries than one chunk holds)
    fleet.setCapacity(0, 1, 1, 1, member=small)
    r = fleet.plan(case.starts(True), case.goals(True))
    assert r[small].status == _capi.PLAN_POOL_FULL and not fleet.initialized(small)
    others = [i for i in range(case.n) if i != small]
    check_fleet(case, fleet, r, st, others)
    assert all(fleet.initialized(i) for i in others)
    fleet.setCapacity(0, *case.cap, member=small)
    r = fleet.plan(case.starts(True), case.goals(True))
    assert fleet.stats() == [case.n - 1, 1, 1, 0]
    assert fleet.initialized(small)
    compare_member(case, case.L[small], fleet.member(small), r[small], st[small])
    st2 = case.o_plan(members=others)  # (a repair with nothing to do)
    check_fleet(case, fleet, r, st2, others)


def driver_map():
    """the map tests/cpp/lpa_fleet_driver.cpp builds"""
    grid = np.zeros((1, 120, 160), dtype=np.int8)
    grid[0, 0:70, 50:55] = 100
    grid[0, 50:120, 100:105] = 100
    return grid, (0.0, 0.0, 0.0), 0.1


DRIVER_PAIRS = [(10, 10, 150, 100), (150, 20, 10, 110), (20, 100, 140, 10), (80, 10, 80, 110)]


@pytest.mark.gpu
def test_fleet_driver_json_equals_the_python_path(tmp_path):
    from mpl_ros_amd.planner import LpaFleet
    exe = _build_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    last = out.stdout.strip().splitlines()[-1]
    d = json.loads(last[last.index("{"):])
    grid, origin, res = driver_map()
    U = mapgen.control_lattice(1.0, 1, False)
    mu, _ = util.make_gpu(grid, origin, res, U, **KW)
    fleet = LpaFleet(mu, 4)
    fleet.setVmax(2.0); fleet.setAmax(1.0); fleet.setDt(1.0); fleet.setU(U); fleet.setTol(0.5, 1, 1)
    fleet.setCapacity(1, 1 << 17, 1 << 19, 1 << 19)
    cell = lambda ix, iy: util.gpu_wp(((ix + 0.5) * 0.1, (iy + 0.5) * 0.1, 0.025))
    starts = [cell(p[0], p[1]) for p in DRIVER_PAIRS]
    goals = [cell(p[2], p[3]) for p in DRIVER_PAIRS]
    cells = [(x, y, 0) for y in range(55, 60) for x in range(70, 90)]
    assert len(d["steps"]) == 3
    for step in range(3):
        changed = [0] * 4
        if step:
            for x, y, z in cells:
                grid[z, y, x] = 100 if step == 1 else 0
            mu.setMap(origin, (160, 120, 1), grid.ravel(), res)
            changed = fleet.updateBlockedNodes(cells) if step == 1 else fleet.updateClearedNodes(cells)
        r = fleet.plan(starts, goals)
        ds = d["steps"][step]
        assert ds["stats"] == fleet.stats() == ([0, 0, 4, 0] if step == 0 else [4, 1, 0, 0])
        for i in range(4):
            m = ds["members"][i]
            ss = fleet.lpaStateSpace(i)
            assert m["status"] == r[i].status == 0
            assert m["cost_bits"] == int(np.float64(r[i].cost).view(np.uint64))
            assert m["n_expanded"] == r[i].n_expanded and m["expand_hash"] == r[i].expand_hash
            assert m["n_nodes"] == r[i].n_nodes and m["n_edges"] == r[i].n_edges and m["traj_len"] == r[i].traj_len
            assert m["changed"] == changed[i] and m["initialized"] == 1
            assert m["space_nodes"] == ss["n_nodes"] and m["blocked_log"] == ss["n_blocked_log"]
        if step == 1:
            assert sum(1 for m in ds["members"] if m["n_expanded"] > 0) >= 1 and all(c > 0 for c in changed)
