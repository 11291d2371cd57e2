"""Host mirror of the reference's 3-D moving-obstacle planner, PolyMapPlanner3D (poly_map_planner.h:107), over the C-ABI
(mplx_poly3_*).  The 2-D interface (poly_map.py) one for one, with 3-D worlds: a `PolyWorld3D` is what one planner sees --
setMap(ori, dim) with the six-face bounding box of poly_map_util.h:52-68, setStartTime, static / linear / nonlinear
obstacles -- and a `PolyTeam3D` holds several worlds on the device so that many queries plan in one launch.  No compute
happens here.
"""
import ctypes as C

import numpy as np

from . import _capi, plpa_space
from ._capi import MplxError

VEL, ACC, JRK, SNP = _capi.VEL, _capi.ACC, _capi.JRK, _capi.SNP


def box(hx, hy=None, hz=None):
    """Polyhedron3D of an axis-aligned box with half sizes (hx, hy, hz) around the origin: rows {px, py, pz, nx, ny, nz}"""
    hy = hx if hy is None else hy
    hz = hx if hz is None else hz
    return np.array([[-hx, 0, 0, -1, -0.0, -0.0], [hx, 0, 0, 1, 0, 0], [0, -hy, 0, -0.0, -1, -0.0], [0, hy, 0, 0, 1, 0],
                     [0, 0, -hz, -0.0, -0.0, -1], [0, 0, hz, 0, 0, 1]], dtype=np.float64)


def control_lattice(u=1.0, num=1, u_z=None):
    """U (n_u x 3): every axis from -u to u in steps of u / num, the loop variable accumulating the step as the nodes' for
    loops do (dz from -u_z to u_z; u_z = 0: planar inputs)"""
    def axis(m):
        if m == 0:
            return [0.0]
        d, vals, x = m / num, [], -m
        while x <= m:
            vals.append(x)
            x += d
        return vals
    zs = axis(u if u_z is None else u_z)
    return np.array([(x, y, z) for x in axis(u) for y in axis(u) for z in zs], dtype=np.float64)


class StaticObstacle3D:        # PolyhedronObstacle3D(poly, p)
    def __init__(self, poly, p):
        self.poly, self.p = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 6), np.array(p, dtype=np.float64)


class LinearObstacle3D:        # PolyhedronLinearObstacle3D(poly, p, v) + set_cov_v
    def __init__(self, poly, p, v, cov_v=0.0):
        self.poly, self.p, self.v, self.cov_v = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 6), np.array(p, float), np.array(v, float), float(cov_v)


class NonlinearObstacle3D:     # PolyhedronNonlinearObstacle3D(poly, traj, t) + disappear_front_/back_
    def __init__(self, poly, segs, start_t, disappear_front=False, disappear_back=False):
        """segs: rows {cx[6], cy[6], cz[6], T} -- the primitives of the obstacle's trajectory"""
        self.poly = np.ascontiguousarray(poly, dtype=np.float64).reshape(-1, 6)
        self.segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 19)
        self.start_t, self.disappear_front, self.disappear_back = float(start_t), bool(disappear_front), bool(disappear_back)


class PolyWorld3D:
    def __init__(self, ori, dim, start_t=0.0):
        self.ori, self.dim, self.start_t = np.array(ori, float), np.array(dim, float), float(start_t)
        self.static, self.linear, self.nonlinear = [], [], []


def acc_segs(p0, v0, us, dt):
    """Trajectory of ACC primitives from (p0, v0) under the inputs `us` (n x 3): rows {cx[6], cy[6], cz[6], T}"""
    p, v = np.array(p0, float), np.array(v0, float)
    rows = []
    for u in us:
        u = np.array(u, float)
        rows.append(sum(([0, 0, 0, u[k], v[k], p[k]] for k in range(3)), []) + [dt])
        p = u / 2 * dt * dt + v * dt + p
        v = u * dt + v
    return np.array(rows).reshape(-1, 19)


def jrk_segs(p0, v0, a0, us, dt):
    """Trajectory of JRK primitives from (p0, v0, a0) under the jerk inputs `us` (cubic segments): rows {cx[6], cy[6], cz[6], T}"""
    p, v, a = np.array(p0, float), np.array(v0, float), np.array(a0, float)
    rows = []
    for u in us:
        u = np.array(u, float)
        rows.append(sum(([0, 0, u[k], a[k], v[k], p[k]] for k in range(3)), []) + [dt])
        p = u / 6 * dt ** 3 + a / 2 * dt * dt + v * dt + p
        v = u / 2 * dt * dt + a * dt + v
        a = u * dt + a
    return np.array(rows).reshape(-1, 19)


U27 = control_lattice(1.0, 1)  # the 27-input lattice: every axis -1, 0, 1

# (centre at t = 0, velocity) of the moving cubes of replanner_world3
REPLANNER_OBS3 = [((6, 12, 1.5), (0, -0.6, 0)), ((10, 6, 2.5), (0, 0.5, 0)), ((13, 14, 2), (-0.3, -0.7, 0)), ((16, 9, 1.25), (0, 0.4, 0.1)),
                  ((8, 9.5, 2.75), (0.4, 0.0, -0.1))]


def replanner_world3(t, turn=False):
    """Synthetic 3-D world of the replanner flow (setLinearObstacles(obstacles as they are at t) + setStartTime(t) per replan), seen
    at time t: a 20 m x 20 m x 4 m box with five 2 m cubes moving at constant velocity (PolyhedronLinearObstacle3D, cov_v 0.2).  The
    box is low enough for the cubes to matter and high enough to pass over or under them.  turn: from t = 2 on the last cube moves
    the other way and the second one stops -- primitives the planner had found free get blocked, blocked ones get free.
    Start / goal: replanner_endpoints3()."""
    W = PolyWorld3D((0.0, 0.0, 0.0), (20.0, 20.0, 4.0), start_t=t)
    cube = box(1.0)
    for k, (p, v) in enumerate(REPLANNER_OBS3):
        p, v = np.array(p, float), np.array(v, float)
        pos = p + v * t
        if turn and t >= 2.0:
            if k == 4:
                pos = p + v * 2.0 - v * (t - 2.0)
                v = -v
            if k == 1:
                pos = p + v * 2.0
                v = 0 * v
        W.linear.append(LinearObstacle3D(cube, pos, v, cov_v=0.2))
    return W


def replanner_endpoints3():
    start = np.zeros(13); start[0], start[1], start[2] = 4.0, 10.0, 2.0
    goal = np.zeros(13); goal[0], goal[1], goal[2] = 19.0, 10.0, 2.0
    return start, goal


class PolyLpa3D:
    """PolyMapPlanner3D with setLPAstar(true): a device-resident LPA* state space over the 3-D moving-obstacle environment of ONE
    world of a PolyTeam3D (mplx_plpa3_*).  PolyLpa (poly_map.py) one for one, states of 13 doubles (pos3 vel3 acc3 jrk3 t).  The flow
    of the replanner node: team.set_worlds(...) (setLinearObstacles, setStartTime) -> update_nodes() -> plan(start, goal) ->
    sub_state_space(1)."""

    def __init__(self, team, world=0, handle=None):
        """handle: a borrowed mplx_plpa3 (a fleet's member, PolyLpaFleet3D.member): a view that does not own it"""
        self.team, self.lib, self.world = team, team.lib, int(world)
        self.result = None
        self.h = None
        self.owned = handle is None
        if handle is not None:
            self.h = C.c_void_p(handle)
            return
        h = C.c_void_p()
        code = self.lib.mplx_plpa3_create(team.h, C.byref(h))
        if code != _capi.OK:
            raise MplxError(f"mplx_plpa3_create failed ({code})")
        self.h = h

    def __del__(self):
        try:
            if self.h and self.owned:
                self.lib.mplx_plpa3_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def check(self, code):
        if code != _capi.OK:
            raise MplxError(f"mplx error {code}: {self.lib.mplx_plpa3_last_error(self.h).decode()}")

    def set_capacity(self, nodes, edges, open_log):
        self.check(self.lib.mplx_plpa3_set_capacity(self.h, int(nodes), int(edges), int(open_log)))

    def initialized(self):
        return bool(self.lib.mplx_plpa3_initialized(self.h))

    def reset(self):
        self.check(self.lib.mplx_plpa3_reset(self.h))

    def plan(self, start, goal, eps=1.0, tol_pos=0.5, tol_vel=-1.0, max_expand=-1, heur_ignore_dynamics=True):
        s = np.ascontiguousarray(start, dtype=np.float64); g = np.ascontiguousarray(goal, dtype=np.float64)
        assert s.size == 13 and g.size == 13, "states are pos3 vel3 acc3 jrk3 t"
        R = _capi.Result()
        self.result = None
        self.check(self.lib.mplx_plpa3_plan(self.h, self.world, s.ctypes.data, g.ctypes.data, float(eps), float(tol_pos), float(tol_vel), int(max_expand),
                                            int(bool(heur_ignore_dynamics)), C.byref(R)))
        self.result = R
        return R.status == _capi.PLAN_OK

    def changed(self):
        """[(entry, now blocked)] of the last updateNodes, by entry number"""
        n = C.c_uint64()
        self.check(self.lib.mplx_plpa3_changed(self.h, 0, None, None, C.byref(n)))
        e = np.zeros(max(n.value, 1), dtype=np.int32); b = np.zeros(max(n.value, 1), dtype=np.int32)
        self.check(self.lib.mplx_plpa3_changed(self.h, n.value, e.ctypes.data, b.ctypes.data, C.byref(n)))
        return list(zip(e[:n.value].tolist(), b[:n.value].tolist()))

    def update_nodes(self):
        """PolyMapPlanner::updateNodes -> (entries that became blocked, entries that became free, [(entry, now blocked)] by entry number)"""
        nb, nc = C.c_uint64(), C.c_uint64()
        self.check(self.lib.mplx_plpa3_update_nodes(self.h, self.world, C.byref(nb), C.byref(nc)))
        return int(nb.value), int(nc.value), self.changed()

    def sub_state_space(self, time_step):
        self.check(self.lib.mplx_plpa3_sub_state_space(self.h, self.world, int(time_step)))

    def traj(self):
        """(actions, node ids, states (n + 1) x 13) of the last successful plan, start -> goal"""
        n = int(self.lib.mplx_plpa3_traj_len(self.h))
        act = np.zeros(max(n, 1), dtype=np.int32); ids = np.zeros(n + 1, dtype=np.int32); st = np.zeros((n + 1, 13))
        if n:
            self.check(self.lib.mplx_plpa3_result_traj(self.h, act.ctypes.data, ids.ctypes.data, st.ctypes.data))
        return act[:n], ids[:n + 1] if n else ids[:0], st[:n + 1] if n else st[:0]

    def expanded_ids(self):
        cap = int(self.result.n_expanded) if self.result is not None else 0
        ids = np.zeros(max(cap, 1), dtype=np.int32)
        n = C.c_uint32()
        self.check(self.lib.mplx_plpa3_result_expanded(self.h, cap, ids.ctypes.data, C.byref(n)))
        return ids[:n.value]

    def last_kernel_ms(self):
        ms = C.c_float()
        self.check(self.lib.mplx_plpa3_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def state_space(self):
        nn, ne = C.c_uint64(), C.c_uint64()
        self.check(self.lib.mplx_plpa3_counts(self.h, C.byref(nn), C.byref(ne)))
        n, m = int(nn.value), int(ne.value)
        states = np.zeros((max(n, 1), 13)); g = np.zeros(max(n, 1)); rhs = np.zeros(max(n, 1)); h = np.zeros(max(n, 1))
        closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy(); built = closed.copy()
        self.check(self.lib.mplx_plpa3_result_nodes(self.h, max(n, 1), states.ctypes.data, g.ctypes.data, rhs.ctypes.data, h.ctypes.data, closed.ctypes.data,
                                                    opened.ctypes.data, built.ctypes.data))
        child = np.zeros(max(m, 1), dtype=np.int32); parent = child.copy(); action = child.copy(); blocked = child.copy()
        self.check(self.lib.mplx_plpa3_result_entries(self.h, max(m, 1), child.ctypes.data, parent.ctypes.data, action.ctypes.data, blocked.ctypes.data))
        return dict(n_nodes=n, states=states[:n], g=g[:n], rhs=rhs[:n], h=h[:n], closed=closed[:n], opened=opened[:n], built=built[:n],
                    child=child[:m], parent=parent[:m], action=action[:m], blocked=blocked[:m], initialized=self.initialized())

    def space(self):
        """the dict of state_space(), key for key, decoded ON THE DEVICE (mplx_plpa3_export_space / _export_records): only the
        result arrays cross the bus, not the pools"""
        return plpa_space.space(self.lib, "plpa3", 13, self.h, self.initialized())

    def records(self, which=plpa_space.WHICH_ALL):
        """the predecessor entries in creation order -- which: 0 all, 1 valid only, 2 blocked only -- as
        dict(entry, child, parent, action, blocked); entry is the record's row in records(0)"""
        return plpa_space.records(self.lib, "plpa3", self.h, which)

    def changed_primitives(self):
        """what getBlockedPrimitives / getClearedPrimitives are built from, for the entries of the last update_nodes() in the order
        of changed(): (parent states n x 13, actions, now-blocked bits) -- gathered on the device, O(changed)"""
        return plpa_space.changed_primitives(self.lib, "plpa3", 13, self.h)

    def export_ms(self):
        """kernel ms of the last space / records / changed_primitives export that ran on this handle"""
        return plpa_space.export_ms(self.lib, "plpa3", self.h)


class PolyLpaFleet3D:
    """N PolyLpa3D planners on ONE PolyTeam3D (its lattice, limits, worlds and obstacles), member i bound to world world_of[i], whose
    plan(), update_nodes() and sub_state_space() run for all members in one launch each (mplx_plpa3_fleet_*): the fresh plans, the
    repairs and the re-roots of different members side by side -- the multi-robot tick.  Per member every result is what the same
    sequence of calls on a PolyLpa3D gives, bit for bit.  PolyLpaFleet (poly_map.py) one for one, states of 13 doubles."""

    def __init__(self, team, world_of):
        self.team, self.lib = team, team.lib
        self.world_of = [int(w) for w in world_of]
        self.n = len(self.world_of)
        self.h = None
        self.members = []
        w = np.ascontiguousarray(self.world_of, dtype=np.int32)
        h = C.c_void_p()
        code = self.lib.mplx_plpa3_fleet_create(team.h, self.n, w.ctypes.data, C.byref(h))
        if code != _capi.OK:
            raise MplxError(f"mplx_plpa3_fleet_create failed ({code})")
        self.h = h
        self.members = [PolyLpa3D(team, self.world_of[i], handle=self.lib.mplx_plpa3_fleet_member(self.h, i)) for i in range(self.n)]
        self.results = None

    def __del__(self):
        try:
            if self.h:
                for m in self.members:
                    m.h = None
                self.lib.mplx_plpa3_fleet_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def check(self, code):
        if code != _capi.OK:
            raise MplxError(f"mplx error {code}: {self.lib.mplx_plpa3_fleet_last_error(self.h).decode()}")

    def member(self, i):
        """member i as a PolyLpa3D (a view: the fleet owns the handle and the view never destroys it)"""
        return self.members[i]

    def spaces(self, members=None):
        """space() of every member (or of the listed ones, in that order), one launch per pass for all of them
        (mplx_plpa3_export_space_many / _export_records_many) -> one dict per member"""
        idx = list(range(self.n)) if members is None else [int(i) for i in members]
        out, self.last_offsets, self.last_entry_offsets = plpa_space.spaces(self.lib, "plpa3", 13, [self.members[i].h for i in idx],
                                                                             [self.members[i].initialized() for i in idx])
        return out

    def set_capacity(self, nodes, edges, open_log):
        self.check(self.lib.mplx_plpa3_fleet_set_capacity(self.h, int(nodes), int(edges), int(open_log)))

    def set_world(self, i, world):
        self.check(self.lib.mplx_plpa3_fleet_set_world(self.h, int(i), int(world)))
        self.world_of[i] = self.members[i].world = int(world)

    def plan(self, starts, goals, active=None, eps=1.0, tol_pos=0.5, tol_vel=-1.0, max_expand=-1, heur_ignore_dynamics=True):
        """plan() of every (active) member, one launch; starts / goals: n x 13.  Returns the n results (zeroed for inactive members)."""
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(self.n, 13)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(self.n, 13)
        a = None if active is None else np.ascontiguousarray([1 if x else 0 for x in active], dtype=np.int32)
        assert a is None or len(a) == self.n
        R = (_capi.Result * self.n)()
        try:
            self.check(self.lib.mplx_plpa3_fleet_plan(self.h, s.ctypes.data, g.ctypes.data, None if a is None else a.ctypes.data, float(eps), float(tol_pos),
                                                      float(tol_vel), int(max_expand), int(bool(heur_ignore_dynamics)), R))
        finally:
            self.results = [R[i] for i in range(self.n)]
            for i, m in enumerate(self.members):
                if a is None or a[i]:
                    m.result = self.results[i]
        return self.results

    def update_nodes(self):
        """updateNodes of every member that holds a space, one launch -> per member (n_blocked, n_cleared, [(entry, now blocked)])"""
        nb = np.zeros(self.n, dtype=np.uint64); nc = np.zeros(self.n, dtype=np.uint64)
        self.check(self.lib.mplx_plpa3_fleet_update_nodes(self.h, nb.ctypes.data, nc.ctypes.data))
        return [(int(nb[i]), int(nc[i]), self.members[i].changed()) for i in range(self.n)]

    def sub_state_space(self, steps):
        """getSubStateSpace(steps[i]) of member i (an int: of every member; < 0 leaves the member alone), one launch"""
        st = np.ascontiguousarray([int(steps)] * self.n if np.isscalar(steps) else steps, dtype=np.int32)
        assert len(st) == self.n
        self.check(self.lib.mplx_plpa3_fleet_sub_state_space(self.h, st.ctypes.data))

    def stats(self):
        """of the last plan / sub_state_space: [members repaired, search launches, members planned afresh, members skipped]"""
        st = np.zeros(4, dtype=np.uint32)
        self.check(self.lib.mplx_plpa3_fleet_stats(self.h, st.ctypes.data))
        return [int(x) for x in st]

    def last_kernel_ms(self):
        """(kernel ms of the last search launch, of the last updateNodes launch)"""
        a, b = C.c_float(), C.c_float()
        self.check(self.lib.mplx_plpa3_fleet_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


class PolyTeam3D:
    """The 3-D worlds of several planners on the device + the shared planner set-up (setVmax/setAmax/setDt/setU/setW)."""

    def __init__(self, device=0):
        self.lib = _capi.load()
        self.h = C.c_void_p()
        code = self.lib.mplx_poly3_create(device, C.byref(self.h))
        if code != _capi.OK:
            raise MplxError(self.lib.mplx_poly3_last_error(None).decode())
        self.n_u = 0
        self._results = []

    def __del__(self):
        try:
            if self.h:
                self.lib.mplx_poly3_destroy(self.h)
        except Exception:
            pass

    def check(self, code):
        if code != _capi.OK:
            raise MplxError(self.lib.mplx_poly3_last_error(self.h).decode())

    def configure(self, control, U, dt, v_max=-1.0, a_max=-1.0, j_max=-1.0, w=10.0):
        U = np.ascontiguousarray(U, dtype=np.float64).reshape(-1, 3)
        self.n_u = U.shape[0]
        self.check(self.lib.mplx_poly3_config(self.h, int(control), self.n_u, U.ctypes.data, float(dt), float(v_max), float(a_max), float(j_max), float(w)))

    def set_worlds(self, worlds):
        self.check(self.lib.mplx_poly3_begin(self.h, len(worlds)))
        D3 = C.c_double * 3
        for i, W in enumerate(worlds):
            self.check(self.lib.mplx_poly3_set_world(self.h, i, D3(*W.ori), D3(*W.dim), W.start_t))
            for o in W.static:
                self.check(self.lib.mplx_poly3_add_static(self.h, i, len(o.poly), o.poly.ctypes.data, D3(*o.p)))
            for o in W.linear:
                self.check(self.lib.mplx_poly3_add_linear(self.h, i, len(o.poly), o.poly.ctypes.data, D3(*o.p), D3(*o.v), o.cov_v))
            for o in W.nonlinear:
                self.check(self.lib.mplx_poly3_add_nonlinear(self.h, i, len(o.poly), o.poly.ctypes.data, len(o.segs), o.segs.ctypes.data,
                                                             o.start_t, int(o.disappear_front), int(o.disappear_back)))
        self.check(self.lib.mplx_poly3_commit(self.h))

    def get_succ_batch(self, world_of, states):
        """env_poly_map<3>::get_succ for K states (K x 13: pos3 vel3 acc3 jrk3 t); returns K x n_u records."""
        w = np.ascontiguousarray(world_of, dtype=np.int32)
        s = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 13)
        out = (_capi.Poly3Succ * (len(w) * self.n_u))()
        self.check(self.lib.mplx_poly3_get_succ_batch(self.h, len(w), w.ctypes.data, s.ctypes.data, out))
        return out

    def set_capacity(self, n_slots, nodes, edges, open_log):
        self.check(self.lib.mplx_poly3_set_capacity(self.h, int(n_slots), int(nodes), int(edges), int(open_log)))

    def set_deadline(self, seconds):
        self.check(self.lib.mplx_poly3_set_deadline(self.h, float(seconds)))

    def set_record(self, cap):
        self.check(self.lib.mplx_poly3_set_record(self.h, int(cap)))

    def plan_batch(self, world_of, starts, goals, eps=1.0, tol_pos=0.5, tol_vel=-1.0, max_expand=-1, heur_ignore_dynamics=True):
        """PlannerBase::plan for one query per entry, all in one launch; starts / goals: n x 13 (pos3 vel3 acc3 jrk3 t)."""
        w = np.ascontiguousarray(world_of, dtype=np.int32)
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 13)
        g = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 13)
        R = (_capi.Result * len(w))()
        self.check(self.lib.mplx_poly3_plan_batch(self.h, len(w), w.ctypes.data, s.ctypes.data, g.ctypes.data, float(eps), float(tol_pos), float(tol_vel),
                                                  int(max_expand), int(bool(heur_ignore_dynamics)), R))
        self._results = [R[i] for i in range(len(w))]
        return self._results

    def traj(self, q):
        """(actions, node ids, states (n + 1) x 13) of query q of the last batch"""
        r = self._results[q]
        n = r.traj_len if r.status == _capi.PLAN_OK else 0
        act = np.zeros(max(n, 1), dtype=np.int32); ids = np.zeros(n + 1, dtype=np.int32); st = np.zeros((n + 1, 13))
        if n:
            self.check(self.lib.mplx_poly3_result_traj(self.h, q, act.ctypes.data, ids.ctypes.data, st.ctypes.data))
        return act[:n], ids[:n + 1] if n else ids[:0], st[:n + 1] if n else st[:0]

    def nodes(self, q):
        """The state space of query q (getCloseSet / getOpenSet): states (n x 13), g, closed, opened"""
        n = int(self._results[q].n_nodes)
        wps = (_capi.Waypoint * max(n, 1))()
        g = np.zeros(max(n, 1)); closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy()
        self.check(self.lib.mplx_poly3_result_nodes(self.h, q, max(n, 1), wps, g.ctypes.data, closed.ctypes.data, opened.ctypes.data))
        st = np.zeros((n, 13))
        for i in range(n):
            st[i, 0:3], st[i, 3:6], st[i, 6:9], st[i, 9:12], st[i, 12] = wps[i].pos[:], wps[i].vel[:], wps[i].acc[:], wps[i].jrk[:], wps[i].t
        return st, g[:n], closed[:n], opened[:n]

    def plan_epoch(self):
        """plan launches of the handle so far"""
        return int(self.lib.mplx_poly3_plan_epoch(self.h))

    def state_space(self, q):
        """The state space of query q of the last plan_batch, exported on the device (mplx_poly3_result_space / _edges): states n x 13
        (pos3 vel3 acc3 jrk3 t) in id order, g, h, closed / opened flags, and the predecessor records (child, parent, action), children
        in id order, each child's records oldest first.  The names are those of PolyTeam.state_space()."""
        q = int(q)
        n = int(self._results[q].n_nodes)
        states = np.zeros((max(n, 1), 13)); g = np.zeros(max(n, 1)); h = np.zeros(max(n, 1))
        closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy()
        self.check(self.lib.mplx_poly3_result_space(self.h, q, n, states.ctypes.data, g.ctypes.data, h.ctypes.data, closed.ctypes.data, opened.ctypes.data))
        ne = C.c_uint64()
        self.check(self.lib.mplx_poly3_result_edges(self.h, q, 0, None, None, None, C.byref(ne)))
        m = int(ne.value)
        child = np.zeros(max(m, 1), dtype=np.int32); parent = child.copy(); action = child.copy()
        if m:
            self.check(self.lib.mplx_poly3_result_edges(self.h, q, m, child.ctypes.data, parent.ctypes.data, action.ctypes.data, C.byref(ne)))
        return dict(n_nodes=n, states=states[:n], g=g[:n], h=h[:n], closed=closed[:n], opened=opened[:n],
                    child=child[:m], parent=parent[:m], action=action[:m])

    def blocked(self, q):
        """(parent, action) of the successors with cost +inf of the states closed at the end of query q's search, parents in id order,
        actions ascending (mplx_poly3_result_blocked: re-derived on the device; refused once the worlds or the set-up have changed)."""
        q = int(q)
        nb = C.c_uint64()
        self.check(self.lib.mplx_poly3_result_blocked(self.h, q, 0, None, None, C.byref(nb)))
        m = int(nb.value)
        parent = np.zeros(max(m, 1), dtype=np.int32); action = parent.copy()
        if m:
            self.check(self.lib.mplx_poly3_result_blocked(self.h, q, m, parent.ctypes.data, action.ctypes.data, C.byref(nb)))
        return parent[:m], action[:m]

    def space_ms(self):
        """(measurement) kernel ms of the last first pass (nodes + scan), edges pass and blocked pass of the state-space export"""
        ms = (C.c_float * 3)()
        self.check(self.lib.mplx_poly3_result_space_ms(self.h, ms))
        return [float(x) for x in ms]

    def _flag_positions(self, q, want_closed):
        q = int(q)
        n = int(self._results[q].n_nodes)
        states = np.zeros((max(n, 1), 13)); closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy()
        self.check(self.lib.mplx_poly3_result_space(self.h, q, n, states.ctypes.data, None, None, closed.ctypes.data, opened.ctypes.data))
        sel = closed[:n] != 0 if want_closed else (opened[:n] != 0) & (closed[:n] == 0)
        return states[:n][sel][:, 0:3].copy()

    def close_set(self, q):
        """getCloseSet(): positions of the states with the closed flag, in id order"""
        return self._flag_positions(q, True)

    def open_set(self, q):
        """getOpenSet(): positions of the states that are opened and not closed, in id order"""
        return self._flag_positions(q, False)

    def expanded_ids(self, q):
        cap = int(self._results[q].n_expanded)
        ids = np.zeros(max(cap, 1), dtype=np.int32)
        n = C.c_uint32()
        self.check(self.lib.mplx_poly3_result_expanded(self.h, q, cap, ids.ctypes.data, C.byref(n)))
        return ids[:n.value]

    def lpa(self, world=0):
        """A PolyLpa3D on world `world` of this team: the LPA* planner of the replanner flow (setLPAstar(true), updateNodes, getSubStateSpace)."""
        return PolyLpa3D(self, world)

    def lpa_fleet(self, world_of):
        """A PolyLpaFleet3D of len(world_of) LPA* planners on this team, member i on world world_of[i]: their plan(), update_nodes()
        and sub_state_space() run in one launch each."""
        return PolyLpaFleet3D(self, world_of)

    def last_kernel_ms(self):
        ms = C.c_float()
        self.check(self.lib.mplx_poly3_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value
