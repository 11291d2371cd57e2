"""ctypes binding of oracle/_ref/libpolymap_ref.so and oracle/_ref/libpolymap3_ref.so: the reference's own env_poly_map /
PolyMapUtil / collide() compiled from where they lie at Dim = 2 (oracle/ref_stubs/poly_map_ref_api.cpp -> RefWorld) and at
Dim = 3 (oracle/ref_stubs/poly_map3_ref_api.cpp -> RefWorld3D), `make -C oracle ref`.
TEST INFRASTRUCTURE ONLY -- see oracle/mpl_oracle.h."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libpolymap_ref.so")
LIB3_PATH = os.path.join(_HERE, "_ref", "libpolymap3_ref.so")


def available(dim=2):
    """is the compiled reference of that dimension there?  (2: libpolymap_ref.so, 3: libpolymap3_ref.so)"""
    return os.path.exists({2: LIB_PATH, 3: LIB3_PATH}[dim])


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        P, D = C.c_void_p, C.c_double
        L.refpoly_create.restype = P
        L.refpoly_create.argtypes = [D, D, D, D]
        L.refpoly_destroy.argtypes = [P]
        L.refpoly_set_start_time.argtypes = [P, D]
        L.refpoly_clear_obstacles.argtypes = [P]
        L.refpoly_add_static.argtypes = [P, C.c_int, C.c_void_p, D, D]
        L.refpoly_add_linear.argtypes = [P, C.c_int, C.c_void_p, D, D, D, D, D]
        L.refpoly_add_nonlinear.argtypes = [P, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, D, C.c_int, C.c_int]
        L.refpoly_set_env.argtypes = [P, C.c_int, C.c_void_p, D, D, D, D, D]
        L.refpoly_is_inside.argtypes = [P, D, D]
        L.refpoly_is_free_point.argtypes = [P, D, D, D]
        L.refpoly_get_succ.argtypes = [P, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.refpoly_plan.argtypes = [P, C.c_void_p, C.c_void_p, C.c_int, D, D, C.c_int, C.c_int]
        L.refpoly_traj_cost.restype = D
        L.refpoly_set_heuristic.argtypes = [C.c_void_p, C.c_void_p]
        L.refpoly_get_expanded.argtypes = [C.c_void_p]
        L.refpoly_get_traj.argtypes = [C.c_void_p, C.c_void_p]
        L.refpoly_get_node.argtypes = [C.c_int, C.c_void_p, C.POINTER(D), C.POINTER(D)]
        L.refpoly_lpa_plan.argtypes = [P, C.c_void_p, C.c_void_p, C.c_int, D, D, C.c_int, C.c_int]
        L.refpoly_lpa_update_nodes.argtypes = [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.refpoly_lpa_sub_state_space.argtypes = [P, C.c_int, C.c_int, D, D, C.c_int, C.c_int]
        L.refpoly_lpa_cost.restype = D
        L.refpoly_lpa_get_expanded.argtypes = [C.c_void_p]
        L.refpoly_lpa_get_traj.argtypes = [C.c_void_p, C.c_void_p]
        L.refpoly_lpa_get_node.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.refpoly_lpa_get_entries.argtypes = [C.c_void_p] * 4
        L.refpoly_lpa_get_changed.argtypes = [C.c_void_p] * 2
        _lib = L
    return _lib


class RefWorld:
    """One reference PolyMapUtil<2> + env_poly_map<2>, filled from a mpl_ros_amd.poly_map.PolyWorld."""

    def __init__(self, world, control, U, dt, v_max=-1.0, a_max=-1.0, j_max=-1.0, w=10.0):
        L = lib()
        self.L, self.control = L, int(control)
        self.h = L.refpoly_create(float(world.ori[0]), float(world.ori[1]), float(world.dim[0]), float(world.dim[1]))
        L.refpoly_set_start_time(self.h, world.start_t)
        for o in world.static:
            L.refpoly_add_static(self.h, len(o.poly), o.poly.ctypes.data, float(o.p[0]), float(o.p[1]))
        for o in world.linear:
            L.refpoly_add_linear(self.h, len(o.poly), o.poly.ctypes.data, float(o.p[0]), float(o.p[1]), float(o.v[0]), float(o.v[1]), o.cov_v)
        for o in world.nonlinear:
            L.refpoly_add_nonlinear(self.h, len(o.poly), o.poly.ctypes.data, len(o.segs), o.segs.ctypes.data, self.control, o.start_t,
                                    int(o.disappear_front), int(o.disappear_back))
        self.U = np.ascontiguousarray(U, dtype=np.float64).reshape(-1, 2)
        self.env_kw = dict(dt=float(dt), v_max=float(v_max), a_max=float(a_max), j_max=float(j_max), w=float(w))
        self.goal_control = None  # control kind of the goal waypoint (None: that of the search states, as robot.hpp builds it)
        L.refpoly_set_env(self.h, len(self.U), self.U.ctypes.data, float(dt), float(v_max), float(a_max), float(j_max), float(w))

    def reload(self, world):
        """The obstacles moved / the planner's start time changed (poly_map_replanner_node.cpp:123-131: setLinearObstacles, setStartTime)"""
        L = self.L
        L.refpoly_clear_obstacles(self.h)
        L.refpoly_set_start_time(self.h, world.start_t)
        for o in world.static:
            L.refpoly_add_static(self.h, len(o.poly), o.poly.ctypes.data, float(o.p[0]), float(o.p[1]))
        for o in world.linear:
            L.refpoly_add_linear(self.h, len(o.poly), o.poly.ctypes.data, float(o.p[0]), float(o.p[1]), float(o.v[0]), float(o.v[1]), o.cov_v)
        for o in world.nonlinear:
            L.refpoly_add_nonlinear(self.h, len(o.poly), o.poly.ctypes.data, len(o.segs), o.segs.ctypes.data, self.control, o.start_t,
                                    int(o.disappear_front), int(o.disappear_back))

    # ---- LPA* over the compiled reference environment (oracle/ref_stubs/poly_map_ref_api.cpp, one state space per process)
    def lpa_reset(self):
        self.L.refpoly_lpa_reset()

    def lpa_plan(self, start, goal, eps=1.0, tol_pos=0.5, max_expand=-1):
        """PlannerBase::plan with setLPAstar(true) (distance heuristic: setHeurIgnoreDynamics(true))"""
        s = np.ascontiguousarray(start, dtype=np.float64); g = np.ascontiguousarray(goal, dtype=np.float64)
        self._lpa_kw = (float(eps), float(tol_pos), int(max_expand))
        st = self.L.refpoly_lpa_plan(self.h, s.ctypes.data, g.ctypes.data, self.control, float(eps), float(tol_pos), int(max_expand), 1)
        ne, nl = self.L.refpoly_lpa_iterations(), self.L.refpoly_lpa_traj_len()
        ids = np.zeros(max(ne, 1), dtype=np.int32)
        self.L.refpoly_lpa_get_expanded(ids.ctypes.data)
        tn = np.zeros(nl + 1, dtype=np.int32); ta = np.zeros(max(nl, 1), dtype=np.int32)
        if st == 0 and nl:
            self.L.refpoly_lpa_get_traj(tn.ctypes.data, ta.ctypes.data)
        return dict(status=st, expanded=ids[:ne], cost=self.L.refpoly_lpa_cost(), actions=ta[:nl], node_ids=tn[:nl + 1] if nl else tn[:0])

    def lpa_update_nodes(self):
        """PolyMapPlanner::updateNodes -> (entries that became blocked, entries that became free, [(entry, now blocked)] by entry)"""
        nb, nc = C.c_int(), C.c_int()
        self.L.refpoly_lpa_update_nodes(self.h, C.byref(nb), C.byref(nc))
        n = self.L.refpoly_lpa_num_changed()
        e = np.zeros(max(n, 1), dtype=np.int32); b = np.zeros(max(n, 1), dtype=np.int32)
        self.L.refpoly_lpa_get_changed(e.ctypes.data, b.ctypes.data)
        order = np.argsort(e[:n], kind="stable")
        return nb.value, nc.value, list(zip(e[:n][order].tolist(), b[:n][order].tolist()))

    def lpa_sub_state_space(self, k):
        eps, tol_pos, max_expand = self._lpa_kw
        self.L.refpoly_lpa_sub_state_space(self.h, int(k), self.control, eps, tol_pos, max_expand, 1)

    def lpa_state_space(self):
        n, ne = self.L.refpoly_lpa_num_nodes(), self.L.refpoly_lpa_num_entries()
        states = np.zeros((n, 9)); vals = np.zeros((n, 3)); flags = np.zeros((n, 3), dtype=np.int32)
        for i in range(n):
            self.L.refpoly_lpa_get_node(i, states[i].ctypes.data, vals[i].ctypes.data, flags[i].ctypes.data)
        child = np.zeros(max(ne, 1), dtype=np.int32); parent = child.copy(); action = child.copy(); blocked = child.copy()
        self.L.refpoly_lpa_get_entries(child.ctypes.data, parent.ctypes.data, action.ctypes.data, blocked.ctypes.data)
        return dict(n_nodes=n, states=states, g=vals[:, 0], rhs=vals[:, 1], h=vals[:, 2], closed=flags[:, 0], opened=flags[:, 1], built=flags[:, 2],
                    child=child[:ne], parent=parent[:ne], action=action[:ne], blocked=blocked[:ne], initialized=bool(self.L.refpoly_lpa_initialized()))

    def __del__(self):
        try:
            self.L.refpoly_destroy(self.h)
        except Exception:
            pass

    def get_succ(self, state):
        s = np.ascontiguousarray(state, dtype=np.float64)
        n = len(self.U)
        succ = np.zeros((n, 9)); cost = np.zeros(n); act = np.zeros(n, dtype=np.int32)
        k = self.L.refpoly_get_succ(self.h, s.ctypes.data, self.control, succ.ctypes.data, cost.ctypes.data, act.ctypes.data)
        return succ[:k], cost[:k], act[:k]

    def plan(self, start, goal, eps=1.0, tol_pos=0.5, max_expand=-1, heur_ignore_dynamics=True):
        """Best-first search through the reference environment.  heur_ignore_dynamics=False (what robot.hpp:109-122 plans with:
        it calls neither setHeurIgnoreDynamics nor setMaxNum): the dynamics-aware heuristic, evaluated by the CPU oracle's
        orc_heuristic on an orc planner configured with this world's w / v_max and the goal."""
        s = np.ascontiguousarray(start, dtype=np.float64); g = np.ascontiguousarray(goal, dtype=np.float64)
        keep = None
        if not heur_ignore_dynamics:
            from . import orc
            U3 = np.zeros((len(self.U), 3)); U3[:, :2] = self.U
            keep = orc.Planner()
            keep.set_config(self.control, U3, dt=self.env_kw["dt"], v_max=self.env_kw["v_max"], a_max=self.env_kw["a_max"], j_max=self.env_kw["j_max"],
                            w=self.env_kw["w"], eps=eps, tol_pos=tol_pos, heur_ignore_dynamics=False)
            gw = orc.Waypoint()
            gw.pos[0], gw.pos[1] = g[0], g[1]
            gw.vel[0], gw.vel[1] = g[2], g[3]
            gw.acc[0], gw.acc[1] = g[4], g[5]
            gw.control = self.goal_control if self.goal_control is not None else self.control
            keep.set_goal(gw)
            self.L.refpoly_set_heuristic(C.cast(keep.L.orc_heuristic, C.c_void_p), keep.h)
        st = self.L.refpoly_plan(self.h, s.ctypes.data, g.ctypes.data, self.control, float(eps), float(tol_pos), int(max_expand), 1 if heur_ignore_dynamics else 0)
        del keep
        ne, nl = self.L.refpoly_num_expanded(), self.L.refpoly_traj_len()
        ids = np.zeros(max(ne, 1), dtype=np.int32)
        self.L.refpoly_get_expanded(ids.ctypes.data)
        tn = np.zeros(nl + 1, dtype=np.int32); ta = np.zeros(max(nl, 1), dtype=np.int32)
        if st == 0 and nl:
            self.L.refpoly_get_traj(tn.ctypes.data, ta.ctypes.data)
        return dict(status=st, expanded=ids[:ne], n_nodes=self.L.refpoly_num_nodes(), cost=self.L.refpoly_traj_cost(), actions=ta[:nl], node_ids=tn[:nl + 1] if nl else tn[:0])

    def node(self, i):
        s = np.zeros(9); g = C.c_double(); h = C.c_double()
        self.L.refpoly_get_node(int(i), s.ctypes.data, C.byref(g), C.byref(h))
        return s, g.value, h.value


_lib3 = None


def lib3():
    global _lib3
    if _lib3 is None:
        L = C.CDLL(LIB3_PATH)
        P, D, I, V = C.c_void_p, C.c_double, C.c_int, C.c_void_p
        L.refpoly3_create.restype = P
        L.refpoly3_create.argtypes = [V, V]
        L.refpoly3_destroy.argtypes = [P]
        L.refpoly3_set_start_time.argtypes = [P, D]
        L.refpoly3_add_static.argtypes = [P, I, V, V]
        L.refpoly3_add_linear.argtypes = [P, I, V, V, V, D]
        L.refpoly3_add_nonlinear.argtypes = [P, I, V, I, V, I, D, I, I]
        L.refpoly3_commit.argtypes = [P]
        L.refpoly3_set_env.argtypes = [P, I, V, D, D, D, D, D]
        L.refpoly3_is_inside.argtypes = [P, V]
        L.refpoly3_is_free_point.argtypes = [P, V, D]
        L.refpoly3_get_succ.argtypes = [P, V, I, V, V, V]
        L.refpoly3_plan.argtypes = [P, V, V, I, D, D, I, I]
        L.refpoly3_traj_cost.restype = D
        L.refpoly3_set_heuristic.argtypes = [V, V]
        L.refpoly3_get_expanded.argtypes = [V]
        L.refpoly3_get_traj.argtypes = [V, V]
        L.refpoly3_get_node.argtypes = [I, V, C.POINTER(D), C.POINTER(D)]
        _lib3 = L
    return _lib3


def _a(x):
    return np.ascontiguousarray(x, dtype=np.float64)


class RefWorld3D:
    """One reference PolyMapUtil<3> + env_poly_map<3>, filled from a mpl_ros_amd.poly_map3d.PolyWorld3D.  The interface of
    tests/poly_checker.CheckerWorld: get_succ, plan, node; rows are the 3-D layouts (hyperplanes {p3, n3}, segments
    {cx[6], cy[6], cz[6], T}, states pos3 vel3 acc3 jrk3 t)."""

    def __init__(self, world, control, U, dt, v_max=-1.0, a_max=-1.0, j_max=-1.0, w=10.0):
        L = lib3()
        self.L, self.control = L, int(control)
        self.h = L.refpoly3_create(_a(world.ori).ctypes.data, _a(world.dim).ctypes.data)
        L.refpoly3_set_start_time(self.h, world.start_t)
        for o in world.static:
            L.refpoly3_add_static(self.h, len(o.poly), o.poly.ctypes.data, _a(o.p).ctypes.data)
        for o in world.linear:
            L.refpoly3_add_linear(self.h, len(o.poly), o.poly.ctypes.data, _a(o.p).ctypes.data, _a(o.v).ctypes.data, o.cov_v)
        for o in world.nonlinear:
            L.refpoly3_add_nonlinear(self.h, len(o.poly), o.poly.ctypes.data, len(o.segs), o.segs.ctypes.data, self.control, o.start_t,
                                     int(o.disappear_front), int(o.disappear_back))
        L.refpoly3_commit(self.h)
        self.U = _a(U).reshape(-1, 3)
        self.env_kw = dict(dt=float(dt), v_max=float(v_max), a_max=float(a_max), j_max=float(j_max), w=float(w))
        L.refpoly3_set_env(self.h, len(self.U), self.U.ctypes.data, float(dt), float(v_max), float(a_max), float(j_max), float(w))

    def __del__(self):
        try:
            self.L.refpoly3_destroy(self.h)
        except Exception:
            pass

    def is_inside(self, pt):
        return bool(self.L.refpoly3_is_inside(self.h, _a(pt).ctypes.data))

    def is_free(self, pt, t):
        """PolyMapUtil::isFree(pt, t)"""
        return bool(self.L.refpoly3_is_free_point(self.h, _a(pt).ctypes.data, float(t)))

    def get_succ(self, state):
        s = _a(state)
        n = len(self.U)
        succ = np.zeros((n, 13)); cost = np.zeros(n); act = np.zeros(n, dtype=np.int32)
        k = self.L.refpoly3_get_succ(self.h, s.ctypes.data, self.control, succ.ctypes.data, cost.ctypes.data, act.ctypes.data)
        return succ[:k], cost[:k], act[:k]

    def plan(self, start, goal, eps=1.0, tol_pos=0.5, max_expand=-1, heur_ignore_dynamics=True):
        """RefWorld.plan at three dimensions: the dynamics-aware heuristic is the CPU oracle's orc_heuristic, handed over with
        refpoly3_set_heuristic"""
        s, g = _a(start), _a(goal)
        keep = None
        if not heur_ignore_dynamics:
            from . import orc
            keep = orc.Planner()
            keep.set_config(self.control, self.U, dt=self.env_kw["dt"], v_max=self.env_kw["v_max"], a_max=self.env_kw["a_max"], j_max=self.env_kw["j_max"],
                            w=self.env_kw["w"], eps=eps, tol_pos=tol_pos, heur_ignore_dynamics=False)
            gw = orc.Waypoint()
            for i in range(3):
                gw.pos[i], gw.vel[i], gw.acc[i] = g[i], g[3 + i], g[6 + i]
            gw.control = self.control
            keep.set_goal(gw)
            self.L.refpoly3_set_heuristic(C.cast(keep.L.orc_heuristic, C.c_void_p), keep.h)
        st = self.L.refpoly3_plan(self.h, s.ctypes.data, g.ctypes.data, self.control, float(eps), float(tol_pos), int(max_expand), 1 if heur_ignore_dynamics else 0)
        del keep
        ne, nl = self.L.refpoly3_num_expanded(), self.L.refpoly3_traj_len()
        ids = np.zeros(max(ne, 1), dtype=np.int32)
        self.L.refpoly3_get_expanded(ids.ctypes.data)
        tn = np.zeros(nl + 1, dtype=np.int32); ta = np.zeros(max(nl, 1), dtype=np.int32)
        if st == 0 and nl:
            self.L.refpoly3_get_traj(tn.ctypes.data, ta.ctypes.data)
        return dict(status=st, expanded=ids[:ne], n_nodes=self.L.refpoly3_num_nodes(), cost=self.L.refpoly3_traj_cost(), actions=ta[:nl], node_ids=tn[:nl + 1] if nl else tn[:0])

    def node(self, i):
        s = np.zeros(13); g = C.c_double(); h = C.c_double()
        self.L.refpoly3_get_node(int(i), s.ctypes.data, C.byref(g), C.byref(h))
        return s, g.value, h.value
