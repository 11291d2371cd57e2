"""Host mirror of the reference's point-cloud planner (mpl_external_planner/.../ellipsoid_planner/ellipsoid_planner.h:
EllipsoidPlanner + env_cloud) over the C-ABI (mplx_cloud_*), with the setter calls ellipsoid_planner_node.cpp:64-175 makes.

The obstacles are a raw point cloud.  setMap uploads it and the device builds its index; plan() runs PlannerBase::plan's
A* on the device.  States are 13 doubles: pos3 vel3 acc3 jrk3 t.  No compute happens here.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import MplxError

VEL, ACC, JRK, SNP = _capi.VEL, _capi.ACC, _capi.JRK, _capi.SNP


def state13(pos, vel=(0, 0, 0), acc=(0, 0, 0), jrk=(0, 0, 0), t=0.0):
    return np.array(list(pos) + list(vel) + list(acc) + list(jrk) + [t], dtype=np.float64)


def control_lattice(u_max, num, use_3d, u_max_z=1.0):
    """ellipsoid_planner_node.cpp:142-157: inputs (dx, dy, dz), each axis from -u_max to u_max in steps of u_max / num (the
    loop variable accumulates the step, as the node's for loops do); dz = 0 unless use_3d (then steps of u_max_z / num)"""
    def axis(m):
        d, vals, x = m / num, [], -m
        while x <= m:
            vals.append(x)
            x += d
        return vals
    zs = axis(u_max_z) if use_3d else [0.0]
    return np.array([(x, y, z) for x in axis(u_max) for y in axis(u_max) for z in zs], dtype=np.float64)


def _poly(c, t):
    """Primitive1D p, v, a, j at t from the six coefficients, in the shim's expressions (mpl_basis/primitive.h)"""
    return (c[0] / 120 * t * t * t * t * t + c[1] / 24 * t * t * t * t + c[2] / 6 * t * t * t + c[3] / 2 * t * t + c[4] * t + c[5],
            c[0] / 24 * t * t * t * t + c[1] / 6 * t * t * t + c[2] / 2 * t * t + c[3] * t + c[4],
            c[0] / 6 * t * t * t + c[1] / 2 * t * t + c[2] * t + c[3],
            c[0] / 2 * t * t + c[1] * t + c[2])


def prior_from_traj(states, actions, U, control, dt, w, seg_dt=None):
    """P1 of csrc/mplx_cloud.h on the host, from a get_traj() result: the trajectory is Trajectory<3> of the primitives
    Primitive<3>(states[i], U[actions[i]], seg_dt) (seg_dt: the dt of the plan that made it, dt by default) and is sampled as
    env_base::set_prior_trajectory does with the dt and w in force: for (t = 0; t < T; t += dt) {evaluate(t), w (T - t)}.
    Returns {"states": n x 13, "controls": n, "cost_to_go": n}."""
    st = np.asarray(states, dtype=np.float64).reshape(-1, 13)
    U = np.asarray(U, dtype=np.float64).reshape(-1, 3)
    act = [int(a) for a in actions]
    seg_dt = float(dt if seg_dt is None else seg_dt)
    dt, w, kind = float(dt), float(w), int(control) & 15
    if not dt > 0 or not seg_dt > 0:
        raise MplxError("prior_from_traj: dt must be > 0")
    segs = []
    for i, a in enumerate(act):  # Primitive(p, u, t): the coefficients by control kind
        p, v, ac, jk = (st[i, 0:3], st[i, 3:6], st[i, 6:9], st[i, 9:12])
        cs = []
        for k in range(3):
            c = [0.0] * 6
            u = float(U[a, k])
            if kind == VEL:
                c[4], c[5] = u, float(p[k])
            elif kind == ACC:
                c[3], c[4], c[5] = u, float(v[k]), float(p[k])
            elif kind == JRK:
                c[2], c[3], c[4], c[5] = u, float(ac[k]), float(v[k]), float(p[k])
            else:
                c[1], c[2], c[3], c[4], c[5] = u, float(jk[k]), float(ac[k]), float(v[k]), float(p[k])
            cs.append(c)
        segs.append(cs)
    taus = [0.0]
    for _ in segs:
        taus.append(seg_dt + taus[-1])
    T = taus[-1] if segs else 0.0
    out_s, out_c = [], []
    t = 0.0
    while t < T:
        tau = 0.0 if t < 0 else (T if t > T else t)  # Trajectory::evaluate
        for i in range(len(segs)):
            if (taus[i] <= tau < taus[i + 1]) or i + 1 == len(segs):
                x = tau - taus[i]
                vals = [_poly(segs[i][k], x) for k in range(3)]
                out_s.append([vals[k][d] for d in range(4) for k in range(3)] + [t])
                break
        out_c.append(w * (T - t))
        t += dt
    n = len(out_c)
    return {"states": np.array(out_s, dtype=np.float64).reshape(n, 13), "controls": np.full(n, kind, dtype=np.int32),
            "cost_to_go": np.array(out_c, dtype=np.float64)}


def _prior_arrays(prior):
    if prior is None:
        return np.zeros((0, 13)), np.zeros(0, dtype=np.int32), np.zeros(0)
    st = np.asarray(prior["states"], dtype=np.float64).reshape(-1, 13)
    ctl = np.asarray(prior["controls"], dtype=np.int32).reshape(-1)
    ctg = np.asarray(prior["cost_to_go"], dtype=np.float64).reshape(-1)
    if not (len(st) == len(ctl) == len(ctg)):
        raise MplxError("prior table: states, controls and cost_to_go must have one length")
    return st, ctl, ctg


class EllipsoidPlanner:
    """MPL::EllipsoidPlanner(verbose) on the device.  Defaults are PlannerBase's."""

    def __init__(self, verbose=False, device=0):
        self.lib = _capi.load()
        self.h = C.c_void_p()
        if self.lib.mplx_cloud_create(device, C.byref(self.h)) != _capi.OK:
            raise MplxError(self.lib.mplx_cloud_last_error(None).decode())
        self.verbose = verbose
        self.control = ACC
        self.eps, self.v_max, self.a_max, self.j_max, self.dt, self.w = 1.0, -1.0, -1.0, -1.0, 1.0, 10.0
        self.max_num = -1
        self.tol_pos, self.tol_vel, self.tol_acc = 0.5, -1.0, -1.0
        self.heur_ignore_dynamics = False
        self.U = None
        self.have_map = False
        self._last = None
        self._priors = []  # the tables in force on the device (set_priors)

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.mplx_cloud_destroy(self.h)
            self.h = C.c_void_p()

    def check(self, code):
        if code != _capi.OK:
            raise MplxError(f"mplx error {code}: {self.lib.mplx_cloud_last_error(self.h).decode()}")

    # ---- setMap and the setters of PlannerBase
    def set_map(self, obs, r, ori, dim):
        pts = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1, 3))
        o, d = (C.c_double * 3)(*map(float, ori)), (C.c_double * 3)(*map(float, dim))
        self.check(self.lib.mplx_cloud_set_map(self.h, len(pts), pts.ctypes.data if len(pts) else None, float(r), o, d))
        self.have_map = True

    def set_epsilon(self, eps): self.eps = float(eps)
    def set_vmax(self, v): self.v_max = float(v)
    def set_amax(self, a): self.a_max = float(a)
    def set_jmax(self, j): self.j_max = float(j)
    def set_dt(self, dt): self.dt = float(dt)
    def set_w(self, w): self.w = float(w)
    def set_max_num(self, n): self.max_num = int(n)
    def set_heur_ignore_dynamics(self, on): self.heur_ignore_dynamics = bool(on)

    def set_tol(self, tol_pos, tol_vel=-1.0, tol_acc=-1.0):
        self.tol_pos, self.tol_vel, self.tol_acc = float(tol_pos), float(tol_vel), float(tol_acc)

    def set_u(self, U):
        self.U = np.ascontiguousarray(np.asarray(U, dtype=np.float64).reshape(-1, 3))

    def set_control(self, control):
        """the control kind of the search states: start.control of the node (use_pos | use_vel | use_acc = JRK by default,
        SNP with use_jrk; ACC without use_acc)"""
        self.control = int(control)

    def set_prior_trajectory(self, prior):
        """PlannerBase::setPriorTrajectory: `prior` is what prior_from_traj returns (the trajectory sampled with the dt and w
        in force, P1 of csrc/mplx_cloud.h).  It guides every query of the later plans until it is changed; an empty table
        clears it (clear_prior_trajectory).  None, a trajectory that does not exist, is refused."""
        if prior is None:
            raise MplxError("EllipsoidPlanner.set_prior_trajectory: prior trajectories are not supported by the device back-end")
        self.set_priors([prior])

    def clear_prior_trajectory(self):
        self.set_priors([])

    def set_priors(self, priors):
        """mplx_cloud_set_prior: no table (clears), one table for every query, or one per query of the next batches (None or
        an empty table: no prior for that query)"""
        tabs = [_prior_arrays(p) for p in priors]
        if len(tabs) == 1 and len(tabs[0][1]) == 0:
            tabs = []
        self._send_priors(tabs)
        self._priors = tabs

    def _send_priors(self, tabs):
        if not tabs:
            self.check(self.lib.mplx_cloud_set_prior(self.h, 0, None, None, None, None))
            return
        off = np.zeros(len(tabs) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(t[1]) for t in tabs])
        st = np.ascontiguousarray(np.concatenate([t[0] for t in tabs]), dtype=np.float64)
        ctl = np.ascontiguousarray(np.concatenate([t[1] for t in tabs]), dtype=np.int32)
        ctg = np.ascontiguousarray(np.concatenate([t[2] for t in tabs]), dtype=np.float64)
        self.check(self.lib.mplx_cloud_set_prior(self.h, len(tabs), off.ctypes.data, st.ctypes.data if len(ctl) else None,
                                                 ctl.ctypes.data if len(ctl) else None, ctg.ctypes.data if len(ctl) else None))

    def heuristic_batch(self, states, goal, set=0):
        """env_base::get_heur (P2) of K states (K x 13, t included) towards `goal` under prior set `set`: the parity entry.
        heur_ignore_dynamics is the one the last plan ran with."""
        self._configure()
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64).reshape(-1, 13))
        g = np.ascontiguousarray(np.asarray(goal, dtype=np.float64).reshape(13))
        h = np.zeros(len(st), dtype=np.float64)
        self.check(self.lib.mplx_cloud_heuristic_batch(self.h, len(st), st.ctypes.data, g.ctypes.data, int(set), h.ctypes.data))
        return h

    def set_lpastar(self, on):
        if on:
            raise MplxError("EllipsoidPlanner.set_lpastar: LPA* is not supported by the point-cloud back-end")

    def _configure(self):
        if self.U is None:
            raise MplxError("EllipsoidPlanner: set_u first")
        if not self.have_map:
            raise MplxError("EllipsoidPlanner: set_map first")
        self.check(self.lib.mplx_cloud_config(self.h, self.control, len(self.U), self.U.ctypes.data, self.dt, self.v_max, self.a_max,
                                              self.j_max, self.w))

    # ---- env_cloud::get_succ (parity entry)
    def get_succ_batch(self, states):
        """states: K x 13.  Returns (valid K x n_u, succ K x n_u x 13, cost K x n_u, action K x n_u)"""
        self._configure()
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64).reshape(-1, 13))
        K, n = len(st), len(self.U)
        out = (_capi.CloudSucc * (K * n))()
        self.check(self.lib.mplx_cloud_get_succ_batch(self.h, K, st.ctypes.data, out))
        a = np.frombuffer(out, dtype=np.dtype([("state", "<f8", 13), ("cost", "<f8"), ("action", "<i4"), ("valid", "<i4")])).reshape(K, n)
        return a["valid"].copy(), a["state"].copy(), a["cost"].copy(), a["action"].copy()

    def last_point_tests(self):
        return int(self.lib.mplx_cloud_last_point_tests(self.h))

    # ---- plan
    def set_capacity(self, n_slots, nodes, edges, open_log):
        self.check(self.lib.mplx_cloud_set_capacity(self.h, n_slots, nodes, edges, open_log))

    def set_deadline(self, seconds):
        self.check(self.lib.mplx_cloud_set_deadline(self.h, float(seconds)))

    def set_record(self, cap):
        self.check(self.lib.mplx_cloud_set_record(self.h, cap))

    def plan_batch(self, starts, goals, priors=None):
        """many queries on the one cloud, one launch: returns the mplx_result dicts.  priors: one table per query (None: no
        prior for that query) for this batch alone; without it the planner's own prior (set_prior_trajectory) guides all"""
        self._configure()
        s = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(-1, 13))
        g = np.ascontiguousarray(np.asarray(goals, dtype=np.float64).reshape(-1, 13))
        if len(s) != len(g):
            raise MplxError("plan_batch: as many goals as starts")
        out = (_capi.Result * len(s))()
        if priors is not None:
            if len(priors) != len(s):
                raise MplxError("plan_batch: as many priors as starts")
            self._send_priors([_prior_arrays(p) for p in priors])
        try:
            code = self.lib.mplx_cloud_plan_batch(self.h, len(s), s.ctypes.data, g.ctypes.data, self.eps, self.tol_pos, self.tol_vel,
                                                  self.tol_acc, self.max_num, int(self.heur_ignore_dynamics), out)
        finally:
            if priors is not None:
                self._send_priors(self._priors)
        self.check(code)
        self._last = [r.as_dict() for r in out]
        return self._last

    def plan(self, start, goal):
        """PlannerBase::plan(start, goal) -> bool"""
        r = self.plan_batch([start], [goal])[0]
        return r["status"] == _capi.PLAN_OK

    def result(self, q=0):
        if self._last is None:
            raise MplxError("no plan yet")
        return self._last[q]

    def get_traj(self, q=0):
        """the trajectory's waypoints (traj_len + 1) x 13 and actions; None when there is none"""
        r = self.result(q)
        n = r["traj_len"]
        if r["status"] != _capi.PLAN_OK or n <= 0:
            return None
        wps, act, ids = (_capi.Waypoint * (n + 1))(), (C.c_int32 * n)(), (C.c_int32 * (n + 1))()
        self.check(self.lib.mplx_cloud_result_traj(self.h, q, wps, act, ids))
        st = np.array([list(w.pos) + list(w.vel) + list(w.acc) + list(w.jrk) + [w.t] for w in wps], dtype=np.float64)
        return {"states": st, "actions": np.array(act[:], dtype=np.int32), "node_ids": np.array(ids[:], dtype=np.int32)}

    def get_traj_cost(self, q=0):
        return self.result(q)["cost"]

    def nodes(self, q=0):
        """(states n x 13, g, closed, opened) of query q's state space"""
        n = self.result(q)["n_nodes"]
        wps = (_capi.Waypoint * max(n, 1))()
        g = np.zeros(max(n, 1), dtype=np.float64)
        cl = np.zeros(max(n, 1), dtype=np.int32)
        op = np.zeros(max(n, 1), dtype=np.int32)
        self.check(self.lib.mplx_cloud_result_nodes(self.h, q, n, wps, g.ctypes.data, cl.ctypes.data, op.ctypes.data))
        st = np.array([list(w.pos) + list(w.vel) + list(w.acc) + list(w.jrk) + [w.t] for w in wps[:n]], dtype=np.float64).reshape(n, 13)
        return st, g[:n], cl[:n].astype(bool), op[:n].astype(bool)

    def state_spaces(self, qs=None):
        """The state spaces of the queries `qs` (None: all) of the last plan_batch, exported on the device in one launch per pass
        (mplx_cloud_result_space*): a dict of numpy arrays, concatenated in the order of qs -- states (n x 13), g, h, closed, opened
        per state, child / parent / action per predecessor record (the query's own node ids; for every state in id order its records
        in arrival order), and node_off / edge_off (len(qs) + 1).  env_cloud skips blocked primitives: every record is a valid one."""
        if self._last is None:
            raise MplxError("no plan yet")
        return _capi.space_export(self.lib, self.h, self.check, "mplx_cloud_result_space", 13, qs, len(self._last))

    def state_space(self, q=0):
        """state_spaces([q]) without the offsets: the state space of one query."""
        st = self.state_spaces([int(q)])
        del st["node_off"], st["edge_off"]
        return st

    def get_close_set(self, q=0):
        st, _, cl, _ = self.nodes(q)
        return st[cl, :3]

    def get_open_set(self, q=0):
        st, _, cl, op = self.nodes(q)
        return st[op & ~cl, :3]

    def get_expanded_nodes(self, q=0):
        """empty, as the reference's (env_cloud.h:57 does not record them)"""
        return np.zeros((0, 3), dtype=np.float64)

    def expanded_ids(self, q=0, cap=1 << 20):
        ids = np.zeros(cap, dtype=np.int32)
        n = C.c_uint32()
        self.check(self.lib.mplx_cloud_result_expanded(self.h, q, cap, ids.ctypes.data, C.byref(n)))
        return ids[:n.value]

    def last_kernel_ms(self):
        ms = C.c_float()
        self.check(self.lib.mplx_cloud_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value
