"""ctypes binding of tests/cpp/poly_lpa_checker.cpp: the CPU checker of the moving-obstacle LPA* at Dim = 2 and 3 (PlannerBase::plan
with setLPAstar(true), PolyMapPlanner::updateNodes, getSubStateSpace over the Env<Dim> of tests/cpp/poly_checker.cpp), compiled with
g++ against include/mpl_shim at first use.  One state space per LpaCheckerWorld; it is a CheckerWorld too (get_succ, the fresh
best-first search `plan`).  The lpa_* methods answer in the shapes of oracle.refpoly.RefWorld's.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import poly_checker
from tests.poly_checker import _a

ROOT = poly_checker.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "poly_lpa_checker.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="poly_lpa_checker_"), "libpolylpachecker.so")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include", "mpl_shim"),
                               "-I", os.path.join(ROOT, "include"), "-o", out, SRC])
        L = C.CDLL(out)
        P, D, I, V = C.c_void_p, C.c_double, C.c_int, C.c_void_p
        # the entries of poly_checker.cpp, which this library holds too
        L.pc_destroy.argtypes = [P]
        L.pc_add_static.argtypes = [P, I, V, V]
        L.pc_add_linear.argtypes = [P, I, V, V, V, D]
        L.pc_add_nonlinear.argtypes = [P, I, V, I, V, I, D, I, I]
        L.pc_set_env.argtypes = [P, I, V, D, D, D, D, D]
        L.pc_get_succ.argtypes = [P, V, I, V, V, V]
        L.pc_is_inside.argtypes = [P, V]
        L.pc_is_free_point.argtypes = [P, V, D]
        L.pc_set_heuristic.argtypes = [V, V]
        L.pc_plan.argtypes = [P, V, V, I, D, D, D, I, I]
        for n in ("pc_num_expanded", "pc_num_nodes", "pc_traj_len"):
            getattr(L, n).argtypes = [P]
        L.pc_traj_cost.argtypes = [P]
        L.pc_traj_cost.restype = D
        L.pc_get_expanded.argtypes = [P, V]
        L.pc_get_traj.argtypes = [P, V, V]
        L.pc_get_node.argtypes = [P, I, V, C.POINTER(D), C.POINTER(D), C.POINTER(I), C.POINTER(I)]
        # the LPA*
        L.plc_create.restype = P
        L.plc_create.argtypes = [I, V, V, D]
        L.plc_clear_obstacles.argtypes = [P, D]
        L.plc_reset.argtypes = [P]
        L.plc_plan.argtypes = [P, V, V, I, D, D, D, I, I]
        L.plc_update_nodes.argtypes = [P, C.POINTER(I), C.POINTER(I)]
        L.plc_sub_state_space.argtypes = [P, I, I, D, D, D, I, I]
        for n in ("plc_initialized", "plc_num_nodes", "plc_num_entries", "plc_iterations", "plc_traj_len", "plc_num_changed"):
            getattr(L, n).argtypes = [P]
        L.plc_cost.argtypes = [P]
        L.plc_cost.restype = D
        L.plc_get_expanded.argtypes = [P, V]
        L.plc_get_traj.argtypes = [P, V, V]
        L.plc_get_node.argtypes = [P, I, V, V, V]
        L.plc_get_entries.argtypes = [P, V, V, V, V]
        L.plc_get_changed.argtypes = [P, V, V]
        _lib = L
    return _lib


class LpaCheckerWorld(poly_checker.CheckerWorld):
    """One checker environment with an LPA* state space of its own, filled from a PolyWorld (Dim 2) or a PolyWorld3D (Dim 3)."""

    def __init__(self, world, control, U, dt, v_max=-1.0, a_max=-1.0, j_max=-1.0, w=10.0):
        L = lib()
        self.L, self.control = L, int(control)
        self.dim = len(world.ori)
        self._keep = []
        ori, dim = _a(world.ori), _a(world.dim)
        self.h = L.plc_create(self.dim, ori.ctypes.data, dim.ctypes.data, float(world.start_t))
        self._fill(world)
        self.U = _a(U).reshape(-1, self.dim)
        self.env_kw = dict(dt=float(dt), v_max=float(v_max), a_max=float(a_max), j_max=float(j_max), w=float(w))
        L.pc_set_env(self.h, len(self.U), self.U.ctypes.data, float(dt), float(v_max), float(a_max), float(j_max), float(w))
        self._lpa_kw = (1.0, 0.5, -1.0, -1, True)

    def _fill(self, world):
        L = self.L
        for o in world.static:
            p = _a(o.p)
            L.pc_add_static(self.h, len(o.poly), o.poly.ctypes.data, p.ctypes.data)
        for o in world.linear:
            p, v = _a(o.p), _a(o.v)
            L.pc_add_linear(self.h, len(o.poly), o.poly.ctypes.data, p.ctypes.data, v.ctypes.data, o.cov_v)
        for o in world.nonlinear:
            L.pc_add_nonlinear(self.h, len(o.poly), o.poly.ctypes.data, len(o.segs), o.segs.ctypes.data, self.control, o.start_t,
                               int(o.disappear_front), int(o.disappear_back))

    def reload(self, world):
        """The obstacles moved / the planner's start time changed (setLinearObstacles, setStartTime); the bounding box stays"""
        self.L.plc_clear_obstacles(self.h, float(world.start_t))
        self._fill(world)

    def _heuristic(self, goal, eps, tol_pos):
        """an orc planner whose orc_heuristic the checker calls (the dynamics-aware heuristic), as CheckerWorld.plan sets one up"""
        from oracle import orc
        U3 = np.zeros((len(self.U), 3)); U3[:, :self.dim] = self.U
        keep = orc.Planner()
        keep.set_config(self.control, U3, dt=self.env_kw["dt"], v_max=self.env_kw["v_max"], a_max=self.env_kw["a_max"], j_max=self.env_kw["j_max"],
                        w=self.env_kw["w"], eps=eps, tol_pos=tol_pos, heur_ignore_dynamics=False)
        gw = orc.Waypoint()
        d = self.dim
        for i in range(d):
            gw.pos[i], gw.vel[i], gw.acc[i] = goal[i], goal[d + i], goal[2 * d + i]
        gw.control = self.control
        keep.set_goal(gw)
        self.L.pc_set_heuristic(C.cast(keep.L.orc_heuristic, C.c_void_p), keep.h)
        return keep

    def lpa_initialized(self):
        return bool(self.L.plc_initialized(self.h))

    def lpa_reset(self):
        self.L.plc_reset(self.h)

    def lpa_plan(self, start, goal, eps=1.0, tol_pos=0.5, tol_vel=-1.0, max_expand=-1, heur_ignore_dynamics=True):
        s, g = _a(start), _a(goal)
        self._lpa_kw = (float(eps), float(tol_pos), float(tol_vel), int(max_expand), bool(heur_ignore_dynamics))
        self._goal = g.copy()
        keep =None if heur_ignore_dynamics else self._heuristic(g, eps, tol_pos)
        st = self.L.plc_plan(self.h, s.ctypes.data, g.ctypes.data, self.control, float(eps), float(tol_pos), float(tol_vel), int(max_expand),
                             1 if heur_ignore_dynamics else 0)
        del keep
        ne, nl = self.L.plc_iterations(self.h), self.L.plc_traj_len(self.h)
        ids = np.zeros(max(ne, 1), dtype=np.int32)
        self.L.plc_get_expanded(self.h, ids.ctypes.data)
        tn = np.zeros(nl + 1, dtype=np.int32); ta = np.zeros(max(nl, 1), dtype=np.int32)
        if st == 0 and nl:
            self.L.plc_get_traj(self.h, tn.ctypes.data, ta.ctypes.data)
        return dict(status=st, expanded=ids[:ne], cost=self.L.plc_cost(self.h), actions=ta[:nl], node_ids=tn[:nl + 1] if nl else tn[:0])

    def lpa_update_nodes(self):
        """PolyMapPlanner::updateNodes -> (entries that became blocked, entries that became free, [(entry, now blocked)] by entry)"""
        nb, nc = C.c_int(), C.c_int()
        self.L.plc_update_nodes(self.h, C.byref(nb), C.byref(nc))
        n = self.L.plc_num_changed(self.h)
        e = np.zeros(max(n, 1), dtype=np.int32); b = np.zeros(max(n, 1), dtype=np.int32)
        self.L.plc_get_changed(self.h, e.ctypes.data, b.ctypes.data)
        order = np.argsort(e[:n], kind="stable")
        return nb.value, nc.value, list(zip(e[:n][order].tolist(), b[:n][order].tolist()))

    def lpa_changed_raw(self):
        """[(entry, now blocked)] of the last updateNodes in the order the walk met them (states in id order, each state's entries oldest first)"""
        n = self.L.plc_num_changed(self.h)
        e = np.zeros(max(n, 1), dtype=np.int32); b = np.zeros(max(n, 1), dtype=np.int32)
        self.L.plc_get_changed(self.h, e.ctypes.data, b.ctypes.data)
        return list(zip(e[:n].tolist(), b[:n].tolist()))

    def lpa_sub_state_space(self, k):
        eps, tol_pos, tol_vel, max_expand, hid = self._lpa_kw
        keep = None if hid else self._heuristic(self._goal, eps, tol_pos)
        self.L.plc_sub_state_space(self.h, int(k), self.control, eps, tol_pos, tol_vel, max_expand, 1 if hid else 0)
        del keep

    def lpa_state_space(self):
        n, ne = self.L.plc_num_nodes(self.h), self.L.plc_num_entries(self.h)
        states = np.zeros((n, self.ns)); vals = np.zeros((n, 3)); flags = np.zeros((n, 3), dtype=np.int32)
        for i in range(n):
            self.L.plc_get_node(self.h, i, states[i].ctypes.data, vals[i].ctypes.data, flags[i].ctypes.data)
        child = np.zeros(max(ne, 1), dtype=np.int32); parent = child.copy(); action = child.copy(); blocked = child.copy()
        self.L.plc_get_entries(self.h, child.ctypes.data, parent.ctypes.data, action.ctypes.data, blocked.ctypes.data)
        return dict(n_nodes=n, states=states, g=vals[:, 0], rhs=vals[:, 1], h=vals[:, 2], closed=flags[:, 0], opened=flags[:, 1], built=flags[:, 2],
                    child=child[:ne], parent=parent[:ne], action=action[:ne], blocked=blocked[:ne], initialized=self.lpa_initialized())
