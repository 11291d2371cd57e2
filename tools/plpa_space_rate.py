"""Numbers of the state-space read-back of the moving-obstacle LPA* planners (no gate): the export on the device
(PolyLpa.space / changed_primitives, PolyLpaFleet3D.spaces: mplx_plpa_export_* / mplx_plpa3_export_*) next to the host-decoded route
(state_space(): two copies of the node pool and one of the entry pool, decoded and list-walked on the host), on
  * the replanner flows of tests/test_poly_lpa.py (2-D) and tests/test_poly3_lpa.py (3-D): ACC, obstacles that change course, 8 ticks
    of update_nodes -> plan -> sub_state_space(1); the space is read after every plan, the changed primitives after every update_nodes;
  * the two fetches of the C++ shim as it would issue them (`shim_space_*`: states + closed + opened + all records, `shim_update_*`:
    parent state, action and now-blocked bit of the changed entries), old route and new;
  * one tick of a 16-member and a 64-member 3-D fleet (the members of tests/test_poly3_lpa_fleet.py, repeated): spaces() in one launch
    per pass against state_space() of one member after the other.
Per figure: wall time (host clock around calls that end in a stream synchronise; median over --reps per tick -- the spaces of a flow
shrink from tick to tick -- and over all ticks x --reps; old and new alternating, after a warm-up of each), kernel time (HIP events around the passes, mplx_plpa_export_ms) and the bytes that cross the bus, computed
from the counts.  usage: python tools/plpa_space_rate.py [--reps N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd import poly_map as pm  # noqa: E402
from mpl_ros_amd import poly_map3d as p3  # noqa: E402

KW = dict(dt=1.0, v_max=2.0, a_max=1.0, w=10.0)
REC_BYTES = 128  # of an ACC state record (160 under JRK)


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def med(x):
    return round(float(np.median(x)), 4) if len(x) else None


class Dim:
    def __init__(self, dim):
        self.dim, self.W, self.prefix = dim, (9 if dim == 2 else 13), ("plpa" if dim == 2 else "plpa3")

    def fn(self, lib, name):
        return getattr(lib, "mplx_%s_%s" % (self.prefix, name))

    # the C++ shim's fetches, issued through the C-ABI as poly2_space_fetch_lpa / PolyMapPlanner::updateNodes issue them
    def shim_space_old(self, l, n, m):
        st = np.zeros((max(n, 1), self.W)); cl = np.zeros(max(n, 1), dtype=np.int32); op = cl.copy()
        e = [np.zeros(max(m, 1), dtype=np.int32) for _ in range(4)]
        l.check(self.fn(l.lib, "result_nodes")(l.h, n, st.ctypes.data, None, None, None, cl.ctypes.data, op.ctypes.data, None))
        l.check(self.fn(l.lib, "result_entries")(l.h, m, *[x.ctypes.data for x in e]))
        return st, cl, op, e

    def shim_space_new(self, l, n, m):
        st = np.zeros((max(n, 1), self.W)); cl = np.zeros(max(n, 1), dtype=np.int32); op = cl.copy()
        e = [np.zeros(max(m, 1), dtype=np.int32) for _ in range(4)]
        cnt = C.c_uint64()
        l.check(self.fn(l.lib, "export_space")(l.h, n, st.ctypes.data, None, None, None, cl.ctypes.data, op.ctypes.data, None, C.byref(cnt)))
        l.check(self.fn(l.lib, "export_records")(l.h, 0, m, None, *[x.ctypes.data for x in e], C.byref(cnt)))
        return st, cl, op, e

    def shim_update_old(self, l, n, m):
        ch = l.changed()
        st = np.zeros((max(n, 1), self.W)); pa = np.zeros(max(m, 1), dtype=np.int32); ac = pa.copy()
        l.check(self.fn(l.lib, "result_nodes")(l.h, n, st.ctypes.data, None, None, None, None, None, None))
        l.check(self.fn(l.lib, "result_entries")(l.h, m, None, pa.ctypes.data, ac.ctypes.data, None))
        e = np.array([c[0] for c in ch], dtype=np.int64)
        return st[pa[e]], ac[e], np.array([c[1] for c in ch], dtype=np.int32)

    def shim_update_new(self, l, n, m):
        return l.changed_primitives()


def replanner_flow(dim, reps):
    D = Dim(dim)
    world, endpoints = (pm.replanner_world, pm.replanner_endpoints) if dim == 2 else (p3.replanner_world3, p3.replanner_endpoints3)
    team = pm.PolyTeam() if dim == 2 else p3.PolyTeam3D()
    team.configure(pm.ACC, pm.U9 if dim == 2 else p3.U27, **KW)
    team.set_worlds([world(0.0, True)])
    team.set_capacity(1, 1 << 16, 1 << 19, 1 << 19)
    l = team.lpa()
    l.set_capacity(1 << 16, 1 << 20, 1 << 20)
    start, goal = endpoints()
    T = {k: [] for k in ("space", "state_space", "shim_space_new", "shim_space_old", "changed_primitives", "two_dumps", "update_nodes", "plan")}
    K = {k: [] for k in ("space_nodes", "space_records", "changed")}
    sizes, t, per_tick = [], 0.0, []
    for tick in range(8):
        mark = {k: len(v) for k, v in T.items()}
        team.set_worlds([world(t, True)])
        w, upd = wall(l.update_nodes)
        T["update_nodes"].append(w)
        n, m = (lambda s: (s["n_nodes"], len(s["child"])))(l.state_space())
        if l.initialized():
            D.shim_update_new(l, n, m); D.shim_update_old(l, n, m)  # warm-up
            for _ in range(reps):
                w, a = wall(lambda: D.shim_update_new(l, n, m))
                T["changed_primitives"].append(w); K["changed"].append(l.export_ms()[2])
                w, b = wall(lambda: D.shim_update_old(l, n, m))
                T["two_dumps"].append(w)
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
        w, ok = wall(lambda: l.plan(start, goal))
        T["plan"].append(w)
        assert ok
        sx, sh = l.space(), l.state_space()  # warm-up
        assert all(np.array_equal(sx[k], sh[k]) for k in sh if k not in ("n_nodes", "initialized"))
        n, m = sx["n_nodes"], len(sx["child"])
        D.shim_space_new(l, n, m); D.shim_space_old(l, n, m)
        for _ in range(reps):
            T["space"].append(wall(l.space)[0])
            ms = l.export_ms()
            K["space_nodes"].append(ms[0]); K["space_records"].append(ms[1])
            T["state_space"].append(wall(l.state_space)[0])
            T["shim_space_new"].append(wall(lambda: D.shim_space_new(l, n, m))[0])
            T["shim_space_old"].append(wall(lambda: D.shim_space_old(l, n, m))[0])
        sizes.append((n, m, len(upd[2])))
        per_tick.append({k: med(v[mark[k]:]) for k, v in T.items()})
        act, ids, st = l.traj()
        if len(act) <= 2:
            break
        l.sub_state_space(1)
        start = st[1].copy()
        t += 1.0
        start[D.W - 1] = t
    n, m, c = (int(np.median([s[i] for s in sizes])) for i in range(3))
    return {"ticks": len(sizes), "states_entries_changed_per_tick": sizes, "wall_ms_per_tick": per_tick,
            "wall_ms": {k: med(v) for k, v in T.items()}, "kernel_ms": {k: med(v) for k, v in K.items()},
            "bytes_at_median_size": {"space": n * (D.W * 8 + 3 * 8 + 1) + m * 16, "state_space": 2 * n * REC_BYTES + m * 12,
                                     "shim_space_new": n * (D.W * 8 + 1) + m * 16, "shim_space_old": 2 * n * REC_BYTES + m * 12,
                                     "changed_primitives": c * 4 + c * (D.W * 8 + 8), "two_dumps": 2 * n * REC_BYTES + m * 12}}


ACC_PAIRS = [((4, 10, 2), (19, 10, 2)), ((5, 2, 2), (12, 18, 2)), ((2, 9, 1), (15, 9, 3)), ((9, 2, 3), (9, 18, 1))]


def fleet_tick(n_members, reps):
    def state13(p):
        s = np.zeros(13)
        s[0:3] = p
        return s

    members = [(turn, state13(s), state13(g)) for s, g in ACC_PAIRS for turn in (False, True)]
    members = [members[i % len(members)] for i in range(n_members)]
    team = p3.PolyTeam3D()
    team.configure(p3.ACC, p3.U27, **KW)
    team.set_worlds([p3.replanner_world3(0.0, False), p3.replanner_world3(0.0, True)])
    team.set_capacity(1, 1 << 16, 1 << 19, 1 << 19)
    fleet = team.lpa_fleet([int(m[0]) for m in members])
    fleet.set_capacity(1 << 15, 1 << 18, 1 << 18)
    w_plan, res = wall(lambda: fleet.plan(np.stack([m[1] for m in members]), np.stack([m[2] for m in members]), max_expand=5000))
    assert all(r.status == 0 for r in res)
    many = fleet.spaces()  # warm-up
    each = [fleet.member(i).state_space() for i in range(n_members)]
    for a, b in zip(many, each):
        assert all(np.array_equal(a[k], b[k]) for k in b if k not in ("n_nodes", "initialized"))
    T = {"spaces": [], "state_space_each": [], "space_each": []}
    K = {"spaces_nodes": [], "spaces_records": []}
    for _ in range(reps):
        T["spaces"].append(wall(fleet.spaces)[0])
        ms = fleet.member(0).export_ms()
        K["spaces_nodes"].append(ms[0]); K["spaces_records"].append(ms[1])
        T["state_space_each"].append(wall(lambda: [fleet.member(i).state_space() for i in range(n_members)])[0])
        T["space_each"].append(wall(lambda: [fleet.member(i).space() for i in range(n_members)])[0])
    n, m = sum(s["n_nodes"] for s in many), sum(len(s["child"]) for s in many)
    return {"members": n_members, "states": n, "entries": m, "plan_wall_ms": round(w_plan, 3),
            "wall_ms": {k: med(v) for k, v in T.items()}, "kernel_ms": {k: med(v) for k, v in K.items()},
            "bytes": {"spaces": n * (13 * 8 + 3 * 8 + 1) + m * 16 + 64 * n_members * 2, "state_space_each": 2 * n * REC_BYTES + m * 12}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"replanner_2d": replanner_flow(2, a.reps), "replanner_3d": replanner_flow(3, a.reps),
           "fleet3d_16": fleet_tick(16, a.reps), "fleet3d_64": fleet_tick(64, a.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
