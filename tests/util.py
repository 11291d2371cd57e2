"""Shared helpers of the parity tests: build the oracle and the HIP planner on the same inputs."""
import numpy as np

from mpl_ros_amd import mapgen
from oracle import orc


def small_map(n=64, seed=7, occupancy=0.08):
    grid, _ = mapgen.random_box_map((n, n, n), seed=seed, occupancy=occupancy, edge=(2, 8))
    return grid, (0.0, 0.0, 0.0), 0.1


def make_oracle(grid, origin, res, control, U, **kw):
    P = orc.Planner()
    P.set_map(grid, origin, res)
    P.free_unknown()
    P.set_config(control, U, **kw)
    return P


def make_gpu(grid, origin, res, U, v_max=-1.0, a_max=-1.0, j_max=-1.0, dt=1.0, w=10.0, eps=1.0, tol_pos=0.5,
             tol_vel=-1.0, tol_acc=-1.0, max_expand=-1, heur_ignore_dynamics=False, t_max=float("inf"),
             n_slots=1, max_nodes=1 << 20, max_edges=1 << 22, max_log=1 << 21, record=0, spec=-1, yaw_max=-1.0):
    from mpl_ros_amd.planner import VoxelMapPlanner, VoxelMapUtil
    mu = VoxelMapUtil()
    dz, dy, dx = grid.shape
    mu.setMap(origin, (dx, dy, dz), grid.ravel(), res)
    mu.freeUnknown()
    pl = VoxelMapPlanner(False)
    pl.setMapUtil(mu)
    pl.setVmax(v_max); pl.setAmax(a_max); pl.setJmax(j_max); pl.setDt(dt); pl.setW(w); pl.setEpsilon(eps)
    pl.setTol(tol_pos, tol_vel, tol_acc); pl.setMaxNum(max_expand); pl.setHeurIgnoreDynamics(heur_ignore_dynamics)
    pl.setTmax(t_max)
    pl.setYawmax(yaw_max)
    pl.setU(U)
    pl.setCapacity(n_slots, max_nodes, max_edges, max_log)
    pl.setSpeculation(spec)
    if record:
        pl.setRecord(record)
    return mu, pl


def gpu_wp(pos, vel=(0, 0, 0), acc=(0, 0, 0), jrk=(0, 0, 0), control=orc.ACC, t=0.0, yaw=None):
    from mpl_ros_amd.planner import Waypoint3D
    w = Waypoint3D(control)
    if yaw is not None:
        w.use_yaw, w.yaw = True, float(yaw)
    w.pos, w.vel, w.acc, w.jrk = np.array(pos, float), np.array(vel, float), np.array(acc, float), np.array(jrk, float)
    w.t = t
    return w


def expand_hash(ids):
    h = 0
    for i in ids:
        h = (h * 0x100000001B3 + (int(i) + 1)) & ((1 << 64) - 1)
    return h


def random_states(rng, n, control, lo, hi, v_max=2.0, a_max=1.0):
    """n random states (pos uniform in [lo,hi]^3, vel/acc on the 0.1 lattice like search states)."""
    out = []
    for _ in range(n):
        pos = np.round(rng.uniform(lo, hi, 3), 2)
        vel = np.round(rng.uniform(-v_max, v_max, 3), 1)
        acc = np.round(rng.uniform(-a_max, a_max, 3), 1) if control & 4 else np.zeros(3)
        jrk = np.round(rng.uniform(-1, 1, 3), 1) if control & 8 else np.zeros(3)
        out.append((pos, vel, acc, jrk))
    return out


def compare_plan(P, pl, start, goal, control, check_traj=True, yaw=None):
    """Run the same query on the oracle (P) and on the HIP planner (pl); assert bit-exact agreement.
    yaw: (start yaw, goal yaw) makes the states yaw-carrying (use_yaw)."""
    ys, yg = yaw if yaw is not None else (None, None)
    so = orc.waypoint(start[0], vel=start[1], acc=start[2] if len(start) > 2 else (0, 0, 0), control=control, yaw=ys)
    go = orc.waypoint(goal[0], vel=goal[1] if len(goal) > 1 else (0, 0, 0), control=control, yaw=yg)
    P.reset_counters()
    st_o = P.plan(so, go)
    sg = gpu_wp(start[0], vel=start[1], acc=start[2] if len(start) > 2 else (0, 0, 0), control=control, yaw=ys)
    gg = gpu_wp(goal[0], vel=goal[1] if len(goal) > 1 else (0, 0, 0), control=control, yaw=yg)
    ok = pl.plan(sg, gg)
    r = pl.getResult()
    assert r.status == st_o, (r.status, st_o)
    assert ok == (st_o == orc.OK)
    c = P.counters()
    ids_o, _ = P.expanded()
    assert r.n_expanded == c["n_expansions"] == len(ids_o)
    assert r.expand_hash == expand_hash(ids_o)
    assert r.n_nodes == P.num_nodes()
    assert r.n_closed == P.num_closed()
    assert r.voxel_reads == c["n_voxel_reads"]
    assert r.n_succ == c["n_succ"] and r.n_succ_finite == c["n_succ_finite"]
    assert r.n_primitives == c["n_primitives"]
    assert r.n_reopen == c["n_reopen"]
    # the whole state space: predecessor lists (every node, edges in arrival order), g, h, closed flags
    co, po, ao = P.edges()
    cg, pg, ag = pl.getEdges()
    assert r.n_edges == len(co) == len(cg)
    assert np.array_equal(cg, co) and np.array_equal(pg, po) and np.array_equal(ag, ao)
    if r.n_nodes <= 60000:
        _, _, g_g, h_g, closed_g, _ = pl._nodes()
        g_o = np.empty(r.n_nodes); h_o = np.empty(r.n_nodes); closed_o = np.empty(r.n_nodes, dtype=np.int32)
        for i in range(r.n_nodes):
            _, g_o[i], h_o[i], closed_o[i] = P.node(i)
        assert np.array_equal(g_g, g_o) and np.array_equal(h_g, h_o) and np.array_equal(closed_g, closed_o)
    if st_o == orc.OK:
        assert r.cost == P.traj_cost  # bit-exact f64
    else:
        assert np.isinf(r.cost)
    if check_traj and st_o == orc.OK:
        to = P.traj()
        tg = pl.getTraj()
        assert len(tg.segs) == to["n"]
        assert np.array_equal(tg.actions, to["actions"])
        assert np.array_equal(tg.node_ids, to["node_ids"])
        for wg, wo in zip(tg.getWaypoints(), to["wps"]):
            assert wg.control == wo.control
            assert np.array_equal(wg.state(), orc.wp_state(wo, wo.control))  # bit-exact (<= 1e-6 required); yaw included when carried
        for pg, po in zip(tg.segs, to["prs"]):
            for k in range(3):
                assert np.array_equal(pg.coeff(k), np.array(po.c[k][:]))
            assert np.array_equal(pg.pr_yaw(), np.array(po.cyaw[:]))
    return r, c


# ---------------------------------------------------------------------------------------------------------------- map geometries
# Non-cubic, offset maps at several resolutions (tests/test_map_geometry.py).  Each entry: cells per axis, origin, res, the set-up of
# the plans run on it (lattice u, planar or 3-D, limits), occupancy / box edges of the seeded map, and a start / goal pair given as
# fractions of the map's extent.  `f32(x)` is the float32-rounded value a VoxelMap message carries.
def f32(x):
    return float(np.float32(x))


GEOMETRIES = {
    # dx > dy > dz and nb0 > nb1 > nb2 (12, 7, 3), no extent a multiple of 8, all-negative origin off the 0.1 lattice
    "f32_01_neg": dict(dim=(93, 52, 21), origin=(-4.63, -2.57, -1.04), res=f32(0.1), u=1.0, use_3d=True, v_max=2.0, a_max=1.0,
                       occupancy=0.15, edge=(2, 8), seed=29, start=(0.10, 0.15, 0.30), goal=(0.90, 0.85, 0.70)),
    # dx > dy > dz and nb0 > nb1 > nb2 (24, 13, 6), mixed-sign origin, finer than 0.1
    "f32_005_mixed": dict(dim=(187, 101, 45), origin=(-3.13, 1.07, -0.52), res=f32(0.05), u=1.0, use_3d=True, v_max=2.0, a_max=1.0,
                          occupancy=0.15, edge=(4, 16), seed=26, start=(0.10, 0.20, 0.50), goal=(0.90, 0.80, 0.50)),
    # dy > dx > dz, origin tens of metres away (p - origin loses low bits), coarser than 0.1
    "r02_far": dict(dim=(43, 61, 13), origin=(48.37, -37.21, 22.63), res=0.2, u=1.0, use_3d=True, v_max=2.0, a_max=1.0,
                    occupancy=0.22, edge=(1, 4), seed=24, start=(0.15, 0.10, 0.50), goal=(0.85, 0.90, 0.50)),
    # one axis shorter than a brick (5 cells), mixed-sign origin
    "r025_thin": dict(dim=(37, 45, 5), origin=(-2.3, -7.9, 0.11), res=0.25, u=1.0, use_3d=True, v_max=2.0, a_max=1.0,
                      occupancy=0.22, edge=(1, 3), seed=14, start=(0.10, 0.10, 0.50), goal=(0.90, 0.90, 0.50)),
    # dz == 1 through the 3-D VoxelMapUtil (not the OccMap wrapper), planar lattice
    "r015_flat": dict(dim=(67, 41, 1), origin=(-5.02, -3.01, -0.075), res=0.15, u=1.0, use_3d=False, v_max=2.0, a_max=1.0,
                      occupancy=0.16, edge=(1, 5), seed=25, start=(0.10, 0.15, 0.50), goal=(0.90, 0.85, 0.50)),
    # the fine map of the long primitives: n = ceil(max_v dt / res) reaches 350; nb (128, 32, 1), all-negative origin
    "r001_long": dict(dim=(1021, 251, 7), origin=(-5.113, -1.277, -0.0351), res=0.01, u=0.5, use_3d=False, v_max=3.5, a_max=1.0,
                      occupancy=0.22, edge=(10, 60), seed=16, start=(0.08, 0.30, 0.50), goal=(0.92, 0.70, 0.50)),
    # the same map with few obstacles: a robot that sets out at 2.6 m/s (n = 260 and more from the first expansion on) finds its way;
    # used by the plan-level tests of the long primitives only (sweep=False: not part of the per-geometry sweep)
    "r001_sparse": dict(dim=(1021, 251, 7), origin=(-5.113, -1.277, -0.0351), res=0.01, u=0.5, use_3d=False, v_max=3.5, a_max=1.0,
                        occupancy=0.03, edge=(10, 60), seed=34, start=(0.08, 0.30, 0.50), goal=(0.92, 0.70, 0.50), sweep=False),
}
# the geometries on which a swapped extent can only shrink an index (mutation runs): dx > dy > dz and nb0 > nb1 > nb2
ORDERED_GEOMETRIES = ("f32_01_neg", "f32_005_mixed", "r001_long", "r001_sparse")


def bricks_per_axis(dim):
    return tuple((d + 7) // 8 for d in dim)


def geometry_map(dim, origin=(0.0, 0.0, 0.0), res=0.1, occupancy=0.08, seed=7, edge=(2, 8), unknown=0.0):
    """Seeded random-box map of dim = (dx, dy, dz) cells: (grid[z][y][x], origin, res).  unknown: fraction of the free cells set to -1."""
    grid, _ = mapgen.random_box_map(tuple(dim), seed=seed, occupancy=occupancy, edge=edge)
    if unknown > 0:
        rng = np.random.default_rng(seed)
        grid[(rng.random(grid.shape) < unknown) & (grid == 0)] = -1
    return grid, tuple(float(o) for o in origin), float(res)


def geometry_point(g, frac):
    """the point at fractions `frac` of the extent of geometry g (a GEOMETRIES entry), rounded to the millimetre"""
    return tuple(round(g["origin"][i] + frac[i] * g["dim"][i] * g["res"], 3) for i in range(3))


def geometry(name, unknown=0.0, bubbles=True):
    """(grid, origin, res, start, goal, entry) of a named geometry; free bubbles around start and goal"""
    g = GEOMETRIES[name]
    grid, origin, res = geometry_map(g["dim"], g["origin"], g["res"], g["occupancy"], g["seed"], g["edge"], unknown)
    start, goal = geometry_point(g, g["start"]), geometry_point(g, g["goal"])
    if bubbles:
        r = max(2, int(round(0.3 / res)))
        mapgen.carve_bubble(grid, start, origin, res, r)
        mapgen.carve_bubble(grid, goal, origin, res, r)
    return grid, origin, res, start, goal, g


def geometry_lattice(g, num=1):
    return mapgen.control_lattice(g["u"], num, g["use_3d"])


def succ_reads(P, cur, U, actions, dt=1.0):
    """Per successor of get_succ(cur): (voxel reads, sample count n) from the oracle alone -- the primitive of each action is built
    and traversed again on its own (orc_is_free_primitive counts a read for every sample inside the map, up to and including an
    occupied one).  Leaves P's counters reset."""
    L = orc.lib()
    out = []
    for a in actions:
        pr = orc.Primitive()
        u = (orc.C.c_double * 3)(*[float(x) for x in U[int(a)][:3]])
        L.orc_primitive_build(orc.C.byref(cur), u, float(dt), orc.C.byref(pr))
        P.reset_counters()
        L.orc_is_free_primitive(P.h, orc.C.byref(pr))
        out.append((P.counters()["n_voxel_reads"], primitive_samples(pr, P._origin_res[1])))
    P.reset_counters()
    return out


def primitive_samples(pr, res):
    """n of the collision test of a primitive: ceil(max_v t / res) (sample times i t / n, i = 0..n)"""
    L = orc.lib()
    max_v = max(L.orc_primitive_max_vel(orc.C.byref(pr), ax) for ax in range(3))
    return int(np.ceil(max_v * pr.t / res))


def node_samples(P, cur, U, dt=1.0):
    """sample counts n of the valid primitives of state `cur` (what one expansion tests), from the oracle alone"""
    L = orc.lib()
    out = []
    for row in U:
        pr = orc.Primitive()
        L.orc_primitive_build(orc.C.byref(cur), (orc.C.c_double * 3)(*[float(x) for x in row[:3]]), float(dt), orc.C.byref(pr))
        if L.orc_validate_primitive(orc.C.byref(pr), P.cfg.v_max, P.cfg.a_max, P.cfg.j_max):
            out.append(primitive_samples(pr, P._origin_res[1]))
    return out


def expanded_samples(P, U, dt=1.0, limit=400):
    """node_samples of (up to `limit`, evenly spaced) states the oracle's last plan expanded"""
    ids, _ = P.expanded()
    step = max(1, len(ids) // limit)
    out = []
    for i in ids[::step]:
        w = P.node(int(i))[0]
        w.control = P.cfg.control
        out.append(node_samples(P, w, U, dt))
    return out


def compare_succ(P, out, states, control, U, dt=1.0, per_succ_reads=False):
    """getSuccBatch output `out` of the states (pos, vel, acc, jrk; node k at t = 0.5 k) against the oracle's get_succ, bit for bit:
    actions, costs, successor states, keys, and the voxel reads -- their total, and with per_succ_reads every successor's own.
    Returns per state [(action, cost, reads, n)] ((action, cost) without per_succ_reads)."""
    nU = U.shape[0]
    total_reads = 0
    info = []
    P.reset_counters()
    reads_o = 0
    for k, (p, v, a, j) in enumerate(states):
        cur = orc.waypoint(p, v, a, j, control, t=0.5 * k)
        succ, cost, act = P.get_succ(cur)
        got = [out[k * nU + i] for i in range(nU)]
        got_valid = [g for g in got if g.valid]
        assert [g.action for g in got_valid] == list(act)
        for g, so, co in zip(got_valid, succ, cost):
            assert g.cost == co or (np.isinf(g.cost) and np.isinf(co))
            assert np.array_equal(np.array(g.wp.pos[:]), np.array(so.pos[:]))
            assert np.array_equal(np.array(g.wp.vel[:]), np.array(so.vel[:]))
            assert np.array_equal(np.array(g.wp.acc[:]), np.array(so.acc[:]))
            assert np.array_equal(np.array(g.wp.jrk[:]), np.array(so.jrk[:]))
            assert g.wp.t == so.t
            key = (orc.C.c_int32 * 13)()
            so.control = control
            nk = orc.lib().orc_waypoint_key(orc.C.byref(so), key)
            assert g.nkey == nk and list(g.key[:nk]) == list(key[:nk])
        total_reads += sum(g.voxel_reads for g in got_valid)
        if per_succ_reads:
            reads_o += P.counters()["n_voxel_reads"]
            rn = succ_reads(P, cur, U, act, dt)
            assert [g.voxel_reads for g in got_valid] == [r for r, _ in rn], (k, p, v)
            info.append([(int(ai), float(co), r, n) for ai, co, (r, n) in zip(act, cost, rn)])
        else:
            info.append([(int(ai), float(co)) for ai, co in zip(act, cost)])
    if not per_succ_reads:
        reads_o = P.counters()["n_voxel_reads"]
    assert total_reads == reads_o
    return info


def aux_of(mu):
    """the context's auxiliary map (search region / potential) as a flat int8 array"""
    out = np.empty(int(np.prod(mu._dim)), dtype=np.int8)
    mu.ctx.check(mu.ctx.lib.mplx_aux_get(mu.ctx.h, out.ctypes.data))
    return out


def disc_offsets(rn, hn):
    """the dilation neighbourhood of the reference node (map_planner_node.cpp:75-83): a disc of rn cells, hn layers up and down"""
    ns = []
    for nx in range(-rn, rn + 1):
        for ny in range(-rn, rn + 1):
            if np.hypot(nx, ny) > rn:
                continue
            for nz in range(-hn, hn + 1):
                if nx == 0 and ny == 0 and nz == 0:
                    continue
                ns.append((nx, ny, nz))
    return np.array(ns, dtype=np.int32)


def compare_map_helpers(P, mu, grid, cells, rays, points):
    """MapUtil helpers of the HIP path (mu) against the oracle (P, same map, unknown cells kept): the three clouds (order and values),
    dilate with the disc and a 3-D neighbourhood, cellStates of `cells`, rayTrace of `rays` ((a, b) pairs), query of `points`."""
    for which, fn in ((0, mu.getCloud), (1, mu.getFreeCloud), (2, mu.getUnknownCloud)):
        a, b = fn(), P.cloud(which)
        assert a.shape == b.shape and np.array_equal(a, b)
    for offs in (disc_offsets(2, 0), disc_offsets(1, 1)):
        mu.dilate(offs)
        P.dilate(offs)
        assert np.array_equal(mu.getMap().reshape(grid.shape), P.get_map())
    st = mu.cellStates(cells)
    assert st.tolist() == [P.cell_state(c) for c in cells]
    for a, b in rays:
        assert np.array_equal(mu.rayTrace(a, b), P.ray_trace(a, b))
    # (after the dilation: the bitmap was rebuilt)
    cells0, st0 = mu.query(points)
    assert [tuple(c) for c in cells0.tolist()] == [P.float_to_int(p) for p in points]
    assert st0.tolist() == [P.cell_state(c) for c in cells0]


def compare_plan_batch(P, pl, queries, res_b, record, control=orc.ACC):
    """planBatch results res_b of (start, goal) position pairs against the oracle's single plans of the same queries"""
    for q, (s, g) in enumerate(queries):
        st = P.plan(orc.waypoint(s, control=control), orc.waypoint(g, control=control))
        ids_o, _ = P.expanded()
        r = res_b[q]
        assert r.status == st
        assert r.n_expanded == len(ids_o) and r.expand_hash == expand_hash(ids_o)
        assert np.array_equal(pl.getExpandedIds(q), ids_o[:record])
        if st == 0:
            assert r.cost == P.traj_cost
            to, tg = P.traj(), pl.getTraj(q)
            assert np.array_equal(tg.actions, to["actions"]) and np.array_equal(tg.node_ids, to["node_ids"])
