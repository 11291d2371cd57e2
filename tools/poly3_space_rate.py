"""Numbers of the state-space export of the 3-D moving-obstacle A* (no gate): kernel time of the three export passes
(mplx_poly3_result_space / _edges / _blocked: HIP-event times of the first pass with its scan, the edges pass, the blocked pass)
and wall time of the three calls, next to the plan's own kernel time and to the wall time of the host-decoded getter
mplx_poly3_result_nodes (positions and flags only: whole node chunks copied and decoded on the host) on the same plan, on
  * the capped open-box query of tests/test_poly3_space.py (57 k states, 108 k predecessor records: two chunks of each), and
  * an obstacle-dense plan: plan 0 of the scene obs_300 of tests/poly3_scenes.py (300 obstacles of the three kinds).
Medians over --reps fresh plans (a new plan drops the cached export).  usage: python tools/poly3_space_rate.py [--reps N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd import _capi  # noqa: E402
from mpl_ros_amd import poly_map3d as p3  # noqa: E402
from tests import poly3_scenes as ps  # noqa: E402
from tests import test_poly3_space as t3  # noqa: E402


def export(team, r):
    """the three getters of query 0, each timed on its own; returns (kernel ms [3], wall ms [space, edges, blocked], records, blocked)"""
    lib, h = team.lib, team.h
    n, m = int(r.n_nodes), int(r.n_edges)
    states = np.zeros((n, 13)); g = np.zeros(n); hh = np.zeros(n)
    closed = np.zeros(n, dtype=np.int32); opened = closed.copy()
    child = np.zeros(max(m, 1), dtype=np.int32); parent = child.copy(); action = child.copy()
    cnt = C.c_uint64()
    t0 = time.perf_counter()
    team.check(lib.mplx_poly3_result_space(h, 0, n, states.ctypes.data, g.ctypes.data, hh.ctypes.data, closed.ctypes.data, opened.ctypes.data))
    t1 = time.perf_counter()
    team.check(lib.mplx_poly3_result_edges(h, 0, m, child.ctypes.data, parent.ctypes.data, action.ctypes.data, C.byref(cnt)))
    t2 = time.perf_counter()
    team.check(lib.mplx_poly3_result_blocked(h, 0, 0, None, None, C.byref(cnt)))
    nb = int(cnt.value)
    bp = np.zeros(max(nb, 1), dtype=np.int32); ba = bp.copy()
    team.check(lib.mplx_poly3_result_blocked(h, 0, nb, bp.ctypes.data, ba.ctypes.data, C.byref(cnt)))
    t3_ = time.perf_counter()
    return np.array(team.space_ms()), np.array([t1 - t0, t2 - t1, t3_ - t2]) * 1e3, m, nb


def host_nodes(team, r):
    """wall ms of mplx_poly3_result_nodes (the C call alone) on the same plan"""
    n = int(r.n_nodes)
    wps = (_capi.Waypoint * n)()
    g = np.zeros(n); closed = np.zeros(n, dtype=np.int32); opened = closed.copy()
    t0 = time.perf_counter()
    team.check(team.lib.mplx_poly3_result_nodes(team.h, 0, n, wps, g.ctypes.data, closed.ctypes.data, opened.ctypes.data))
    return (time.perf_counter() - t0) * 1e3


def measure(team, world, start, goal, reps, **kw):
    r = team.plan_batch([world], [start], [goal], **kw)[0]  # warm-up
    export(team, r)
    host_nodes(team, r)
    plan_ms, ker, wall, host = [], [], [], []
    for _ in range(reps):
        r = team.plan_batch([world], [start], [goal], **kw)[0]
        plan_ms.append(team.last_kernel_ms())
        k, w, m, nb = export(team, r)
        ker.append(k); wall.append(w)
        host.append(host_nodes(team, r))
    k, w = np.median(np.array(ker), axis=0), np.median(np.array(wall), axis=0)
    return {"status": int(r.status), "n_nodes": int(r.n_nodes), "n_edges": m, "n_blocked": nb, "plan_kernel_ms": float(np.median(plan_ms)),
            "first_pass_ms": float(k[0]), "edges_pass_ms": float(k[1]), "blocked_pass_ms": float(k[2]),
            "space_wall_ms": float(w[0]), "edges_wall_ms": float(w[1]), "blocked_wall_ms": float(w[2]), "three_getters_wall_ms": float(w.sum()),
            "result_nodes_wall_ms": float(np.median(host))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = {}
    s, g = t3.open_query()
    team = t3.make_team(p3.ACC, ps.U27, t3.OPEN_ENV, [t3.open_world()])
    out["open_box_capped"] = measure(team, 0, s, g, a.reps, eps=0.0, max_expand=t3.CHUNK_CAP)
    S = ps.get("obs_300")
    p = S.plans[0]
    team = t3.make_team(S.control, S.U, S.env, S.worlds)
    out["obs_300_plan_0"] = measure(team, p["world"], p["start"], p["goal"], a.reps, **p["kw"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
