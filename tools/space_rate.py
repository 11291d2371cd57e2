"""Numbers of the state-space export over a list of queries (mplx_result_space* / mplx_cloud_result_space*, no gate): HIP-event kernel
time of the passes and host wall time of the calls, each the median of --reps repetitions after a warm-up, on
  (a) the BASELINE C2 single query (mapgen.benchmark_map(256), the 27-input ACC lattice, the set-up of tools/ab.py's c2 leg): the
      host-decoded getters mplx_result_nodes + mplx_result_edges against the export (states, then records) of the same plan;
  (b) the 64-query JRK batch on the office cloud, cap 3000 (the batch of tools/cloud_prior_rate.py, no prior): a loop of
      mplx_cloud_result_nodes over the 64 queries (positions, g and flags only: no h, no records), 64 one-query exports (states and
      records each), and one 64-query export.
A fresh plan precedes every repetition of an export (a new plan drops the cached passes).  usage: python tools/space_rate.py [--reps N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd import _capi, mapgen  # noqa: E402
from mpl_ros_amd.ellipsoid import JRK, EllipsoidPlanner, control_lattice, state13  # noqa: E402
from tests import cloud_scenes as S  # noqa: E402
from tests import util  # noqa: E402


def ms_of(lib, fn, h):
    ms = (C.c_float * 2)()
    getattr(lib, fn)(h, ms)
    return float(ms[0]), float(ms[1])


def export(lib, h, check, prefix, width, qs):
    """states, then records of the list qs through the raw entry points; returns (kernel ms nodes+scan, kernel ms edges, wall ms states,
    wall ms records, states, records)"""
    qa = np.asarray(qs, dtype=np.int32)
    no, eo = np.zeros(len(qa) + 1, dtype=np.uint64), np.zeros(len(qa) + 1, dtype=np.uint64)
    t0 = time.perf_counter()
    check(getattr(lib, prefix + "_counts")(h, len(qa), qa.ctypes.data, no.ctypes.data, eo.ctypes.data))
    n, m = int(no[-1]), int(eo[-1])
    st, g, hh = np.empty((n, width)), np.empty(n), np.empty(n)
    cl, op = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    check(getattr(lib, prefix)(h, len(qa), qa.ctypes.data, n, st.ctypes.data, g.ctypes.data, hh.ctypes.data, cl.ctypes.data, op.ctypes.data))
    t1 = time.perf_counter()
    c, p, a = (np.empty(m, dtype=np.int32) for _ in range(3))
    check(getattr(lib, prefix + "_edges")(h, len(qa), qa.ctypes.data, m, c.ctypes.data, p.ctypes.data, a.ctypes.data))
    t2 = time.perf_counter()
    k = ms_of(lib, prefix + "_ms", h)
    return k[0], k[1], (t1 - t0) * 1e3, (t2 - t1) * 1e3, n, m


def med(rows):
    return [float(x) for x in np.median(np.array(rows, dtype=np.float64), axis=0)]


def case_c2(reps):
    grid, origin, res, s, t, _ = mapgen.benchmark_map(256)
    U = mapgen.control_lattice(1.0, 1, True)
    mu, pl = util.make_gpu(grid, origin, res, U, max_nodes=1 << 22, max_edges=1 << 24, max_log=1 << 23, v_max=2.0, a_max=1.0, tol_pos=0.5)
    pl.setDeadline(100.0)
    ctx, lib = mu.ctx, mu.ctx.lib
    host, dev = [], []
    for it in range(reps + 1):
        pl.plan(util.gpu_wp(s), util.gpu_wp(t))
        r = pl.getResult()
        n, m = int(r.n_nodes), int(r.n_edges)
        coords = (_capi.Waypoint * max(n, 1))()
        g, h, cl, op = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        c, p, a = (np.empty(max(m, 1), dtype=np.int32) for _ in range(3))
        got = C.c_uint64()
        t0 = time.perf_counter()
        ctx.check(lib.mplx_result_nodes(ctx.h, n, coords, g.ctypes.data, h.ctypes.data, cl.ctypes.data, op.ctypes.data))
        t1 = time.perf_counter()
        ctx.check(lib.mplx_result_edges(ctx.h, c.ctypes.data, p.ctypes.data, a.ctypes.data, m, C.byref(got)))
        t2 = time.perf_counter()
        e = export(lib, ctx.h, ctx.check, "mplx_result_space", 14, [0])
        if it:  # (the first round is the warm-up)
            host.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3])
            dev.append(e[:4])
    hm, dm = med(host), med(dev)
    return {"status": int(r.status), "n_nodes": n, "n_edges": m, "plan_kernel_ms": float(pl.lastKernelMs()),
            "result_nodes_wall_ms": hm[0], "result_edges_wall_ms": hm[1], "host_getters_wall_ms": hm[0] + hm[1],
            "export_nodes_scan_kernel_ms": dm[0], "export_edges_kernel_ms": dm[1], "export_states_wall_ms": dm[2], "export_records_wall_ms": dm[3],
            "export_wall_ms": dm[2] + dm[3]}


def case_cloud(reps):
    L = S.LAUNCH
    pl = EllipsoidPlanner(False)
    pl.set_map(S.office(), L["r"], S.ORI, S.DIM)
    pl.set_control(JRK)
    pl.set_u(control_lattice(L["u_max"], L["num"], False))
    pl.set_dt(L["dt"]); pl.set_vmax(L["v_max"]); pl.set_amax(L["a_max"]); pl.set_w(L["w"])
    pl.set_epsilon(L["eps"]); pl.set_tol(*L["tol"])
    pl.set_max_num(3000)
    pl.set_capacity(64, 1 << 22, 1 << 24, 1 << 23)
    rng = np.random.default_rng(64)
    xs = [7.5, 10.0, 14.0, 16.0, 20.0, 22.0, 26.0, 29.5]
    starts, goals = [], []
    for _ in range(64):
        i, j = rng.choice(len(xs), 2, replace=False)
        starts.append(state13((xs[i], rng.uniform(13.0, 16.0), 1.3)))
        goals.append(state13((xs[j], rng.uniform(13.0, 16.0), 1.3)))
    lib = pl.lib
    loop, singles, many = [], [], []
    for it in range(reps + 1):
        res = pl.plan_batch(starts, goals)
        t0 = time.perf_counter()
        for q in range(64):  # the host-decoded getter, the C call alone
            n = res[q]["n_nodes"]
            wps = (_capi.Waypoint * max(n, 1))()
            g, cl, op = np.empty(max(n, 1)), np.empty(max(n, 1), dtype=np.int32), np.empty(max(n, 1), dtype=np.int32)
            pl.check(lib.mplx_cloud_result_nodes(pl.h, q, n, wps, g.ctypes.data, cl.ctypes.data, op.ctypes.data))
        t1 = time.perf_counter()
        k0 = k1 = 0.0
        for q in range(64):
            e = export(lib, pl.h, pl.check, "mplx_cloud_result_space", 13, [q])
            if res[q]["n_nodes"]:
                k0 += e[0]
                k1 += e[1] if e[5] else 0.0
        t2 = time.perf_counter()
        pl.plan_batch(starts, goals)  # (drops the cached passes of the last single export)
        e = export(lib, pl.h, pl.check, "mplx_cloud_result_space", 13, list(range(64)))
        if it:
            loop.append([(t1 - t0) * 1e3])
            singles.append([k0, k1, (t2 - t1) * 1e3])
            many.append(e[:4])
    lm, sm, mm = med(loop), med(singles), med(many)
    return {"queries": 64, "n_nodes": int(e[4]), "n_edges": int(e[5]), "plan_kernel_ms": float(pl.last_kernel_ms()),
            "result_nodes_loop_wall_ms": lm[0],
            "single_exports_nodes_scan_kernel_ms": sm[0], "single_exports_edges_kernel_ms": sm[1], "single_exports_wall_ms": sm[2],
            "many_export_nodes_scan_kernel_ms": mm[0], "many_export_edges_kernel_ms": mm[1], "many_export_states_wall_ms": mm[2],
            "many_export_records_wall_ms": mm[3], "many_export_wall_ms": mm[2] + mm[3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    print(json.dumps({"c2_single": case_c2(a.reps), "cloud_jrk_64": case_cloud(a.reps)}))


if __name__ == "__main__":
    main()
