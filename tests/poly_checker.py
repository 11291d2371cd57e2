"""ctypes binding of tests/cpp/poly_checker.cpp: the CPU checker of the moving-obstacle environment at Dim = 2 and 3, compiled
with g++ against include/mpl_shim at first use (the basis classes oracle/_ref/libpolymap_ref.so is built against).  Worlds are
mpl_ros_amd.poly_map.PolyWorld (Dim 2) or mpl_ros_amd.poly_map3d.PolyWorld3D (Dim 3); states are pos vel acc jrk (Dim each) t.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "poly_checker.cpp")
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="poly_checker_"), "libpolychecker.so")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include", "mpl_shim"),
                               "-I", os.path.join(ROOT, "include"), "-o", out, SRC])
        L = C.CDLL(out)
        P, D, I, V = C.c_void_p, C.c_double, C.c_int, C.c_void_p
        L.pc_create.restype = P
        L.pc_create.argtypes = [I, V, V, D]
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
        _lib = L
    return _lib


def _a(x):
    return np.ascontiguousarray(x, dtype=np.float64)


class CheckerWorld:
    """One checker environment (PolyMapUtil<Dim> + env_poly_map<Dim>) filled from a 2-D or 3-D world."""

    def __init__(self, world, control, U, dt, v_max=-1.0, a_max=-1.0, j_max=-1.0, w=10.0):
        L = lib()
        self.L, self.control = L, int(control)
        self.dim = len(world.ori)
        self._keep = []
        ori, dim = _a(world.ori), _a(world.dim)
        self.h = L.pc_create(self.dim, ori.ctypes.data, dim.ctypes.data, float(world.start_t))
        for o in world.static:
            p = _a(o.p); self._keep.append(p)
            L.pc_add_static(self.h, len(o.poly), o.poly.ctypes.data, p.ctypes.data)
        for o in world.linear:
            p, v = _a(o.p), _a(o.v); self._keep += [p, v]
            L.pc_add_linear(self.h, len(o.poly), o.poly.ctypes.data, p.ctypes.data, v.ctypes.data, o.cov_v)
        for o in world.nonlinear:
            L.pc_add_nonlinear(self.h, len(o.poly), o.poly.ctypes.data, len(o.segs), o.segs.ctypes.data, self.control, o.start_t,
                               int(o.disappear_front), int(o.disappear_back))
        self.U = _a(U).reshape(-1, self.dim)
        self.env_kw = dict(dt=float(dt), v_max=float(v_max), a_max=float(a_max), j_max=float(j_max), w=float(w))
        L.pc_set_env(self.h, len(self.U), self.U.ctypes.data, float(dt), float(v_max), float(a_max), float(j_max), float(w))

    def __del__(self):
        try:
            self.L.pc_destroy(self.h)
        except Exception:
            pass

    @property
    def ns(self):
        return 4 * self.dim + 1

    def is_inside(self, pt):
        return bool(self.L.pc_is_inside(self.h, _a(pt).ctypes.data))

    def is_free(self, pt, t):
        """PolyMapUtil::isFree(pt, t)"""
        return bool(self.L.pc_is_free_point(self.h, _a(pt).ctypes.data, float(t)))

    def get_succ(self, state):
        s = _a(state)
        n = len(self.U)
        succ = np.zeros((n, self.ns)); cost = np.zeros(n); act = np.zeros(n, dtype=np.int32)
        k = self.L.pc_get_succ(self.h, s.ctypes.data, self.control, succ.ctypes.data, cost.ctypes.data, act.ctypes.data)
        return succ[:k], cost[:k], act[:k]

    def plan(self, start, goal, eps=1.0, tol_pos=0.5, max_expand=-1, heur_ignore_dynamics=True, tol_vel=-1.0):
        """The best-first search of refpoly_plan over this environment.  heur_ignore_dynamics=False: the CPU oracle's
        orc_heuristic on an orc planner configured with this world's w / v_max and the goal (z components zero at Dim 2)."""
        s, g = _a(start), _a(goal)
        keep = None
        if not heur_ignore_dynamics:
            from oracle import orc
            U3 = np.zeros((len(self.U), 3)); U3[:, :self.dim] = self.U
            keep = orc.Planner()
            keep.set_config(self.control, U3, dt=self.env_kw["dt"], v_max=self.env_kw["v_max"], a_max=self.env_kw["a_max"], j_max=self.env_kw["j_max"],
                            w=self.env_kw["w"], eps=eps, tol_pos=tol_pos, heur_ignore_dynamics=False)
            gw = orc.Waypoint()
            d = self.dim
            for i in range(d):
                gw.pos[i], gw.vel[i], gw.acc[i] = g[i], g[d + i], g[2 * d + i]
            gw.control = self.control
            keep.set_goal(gw)
            self.L.pc_set_heuristic(C.cast(keep.L.orc_heuristic, C.c_void_p), keep.h)
        st = self.L.pc_plan(self.h, s.ctypes.data, g.ctypes.data, self.control, float(eps), float(tol_pos), float(tol_vel), int(max_expand),
                             1 if heur_ignore_dynamics else 0)
        del keep
        ne, nl = self.L.pc_num_expanded(self.h), self.L.pc_traj_len(self.h)
        ids = np.zeros(max(ne, 1), dtype=np.int32)
        self.L.pc_get_expanded(self.h, ids.ctypes.data)
        tn = np.zeros(nl + 1, dtype=np.int32); ta = np.zeros(max(nl, 1), dtype=np.int32)
        if st == 0 and nl:
            self.L.pc_get_traj(self.h, tn.ctypes.data, ta.ctypes.data)
        return dict(status=st, expanded=ids[:ne], n_nodes=self.L.pc_num_nodes(self.h), cost=self.L.pc_traj_cost(self.h), actions=ta[:nl],
                    node_ids=tn[:nl + 1] if nl else tn[:0])

    def node(self, i):
        s = np.zeros(self.ns); g = C.c_double(); h = C.c_double(); cl = C.c_int(); op = C.c_int()
        self.L.pc_get_node(self.h, int(i), s.ctypes.data, C.byref(g), C.byref(h), C.byref(cl), C.byref(op))
        return s, g.value, h.value, cl.value, op.value
