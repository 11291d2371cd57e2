"""The voxel planners on non-cubic, offset maps at several resolutions, and on primitives long enough for the generic sampling loop.

Every other GPU test plans on cubes (tests/util.small_map: edge a multiple of 8, origin 0, res 0.1) or on the two fixture maps
(dx == dy, origin >= 0, res float32(0.1)).  Here the maps are util.GEOMETRIES: pairwise different extents, extents that are not
multiples of the brick edge, an axis shorter than a brick, dz == 1 through the 3-D MapUtil, negative / mixed-sign / far-away origins
off the cell lattice, and the resolutions float32(0.1), float32(0.05), 0.2, 0.25, 0.15 and 0.01.  Everything is compared with the
CPU oracle bit for bit (util.compare_plan, util.compare_succ, util.compare_map_helpers, test_lpa.compare_lpa, the fleet helpers of
test_lpa_fleet).  The regimes a test is meant to reach (kinds of blocked successor, samples per primitive, samples per node) are
asserted from the oracle's output alone, before the comparison, so inputs that drift out of a regime fail the test.

CPU part: the table covers what it is meant to cover; the oracle plans are non-trivial and cheap."""
import time

import numpy as np
import pytest

from mpl_ros_amd import mapgen
from oracle import orc
from tests import util
from tests.test_lpa import box_cells, compare_lpa
from tests.test_lpa_fleet import Case, CheckerSide, FleetSide, check_fleet, replay

NAMES = [n for n, g in util.GEOMETRIES.items() if g.get("sweep", True)]
CN = {orc.VEL: "VEL", orc.ACC: "ACC", orc.JRK: "JRK", orc.SNP: "SNP"}
LONG, SPARSE = "r001_long", "r001_sparse"


def plan_kw(g, control, **over):
    kw = dict(v_max=g["v_max"], a_max=g["a_max"], tol_pos=0.5)
    if control in (orc.JRK, orc.SNP):
        kw["j_max"] = 1.0
    kw.update(over)
    return kw


def start_of(control, pos, vel=(0, 0, 0)):
    return (pos, vel, (0, 0, 0)) if control in (orc.JRK, orc.SNP) else (pos, vel)


# ---------------------------------------------------------------------------------------------------------------- CPU: the table
def test_geometry_table_covers_what_the_sweep_is_for():
    G = util.GEOMETRIES
    assert len(G) >= 6
    distinct = [n for n, g in G.items() if len(set(g["dim"])) == 3 and g["dim"][2] > 1]
    assert len(distinct) >= 4
    ordered = [n for n, g in G.items() if g["dim"][0] > g["dim"][1] > g["dim"][2] > 1 and
               util.bricks_per_axis(g["dim"])[0] > util.bricks_per_axis(g["dim"])[1] > util.bricks_per_axis(g["dim"])[2]]
    assert len(ordered) >= 2 and set(ordered) == set(util.ORDERED_GEOMETRIES)
    assert any(g["dim"][1] > g["dim"][0] for g in G.values())  # ... and the other order of x and y
    # partial bricks: extents that 8 does not divide on every axis, an axis shorter than a brick, a single layer
    for ax in range(3):
        assert any(g["dim"][ax] % 8 and g["dim"][ax] > 8 for g in G.values())
    assert any(1 < min(g["dim"]) < 8 for g in G.values())
    assert any(g["dim"][2] == 1 for g in G.values())
    # origins: all negative, mixed sign, tens of metres away; off the cell lattice
    assert any(all(o < 0 for o in g["origin"]) for g in G.values())
    assert any(min(g["origin"]) < 0 < max(g["origin"]) for g in G.values())
    assert any(max(abs(o) for o in g["origin"]) >= 20.0 for g in G.values())
    for g in G.values():
        assert any(abs(o / g["res"] - round(o / g["res"])) > 1e-3 for o in g["origin"])
    # resolutions: the float32-rounded ones a VoxelMap message carries, and exact decimals
    have = {g["res"] for g in G.values()}
    assert {util.f32(0.1), util.f32(0.05), 0.2, 0.25, 0.15, 0.01} <= have
    assert util.f32(0.1) != 0.1 and util.f32(0.05) != 0.05
    # the combination the whole-plan families must see: distinct extents, a partial brick, a negative origin, res != 0.1
    for n in ("f32_005_mixed", LONG):
        g = G[n]
        assert n in distinct and any(d % 8 for d in g["dim"]) and min(g["origin"]) < 0 and abs(g["res"] - 0.1) > 0.01
    # the long-primitive map: a primitive at v_max has more samples than the staged path can index
    g = G[LONG]
    assert g["v_max"] * 1.0 / g["res"] > 300


def test_oracle_plans_on_the_geometries_are_non_trivial_and_cheap():
    t0 = time.time()
    capped = 0
    for name in NAMES:
        grid, origin, res, start, goal, g = util.geometry(name)
        assert grid.shape == g["dim"][::-1]
        U = util.geometry_lattice(g)
        for control in (orc.ACC, orc.JRK):
            P = util.make_oracle(grid, origin, res, control, U, **plan_kw(g, control, max_expand=1500))
            st = P.plan(orc.waypoint(start, control=control), orc.waypoint(goal, control=control))
            n = len(P.expanded()[0])
            assert st in (orc.OK, orc.MAX_EXPAND) and n >= 300, (name, control, st, n)
            capped += st == orc.MAX_EXPAND
    assert capped >= 2 and time.time() - t0 < 20.0


# ---------------------------------------------------------------------------------------------------------------- utilities
def face_points(g, rng):
    """query points: on cell faces (negative cell indices included), just inside / outside the six faces, random ones around the map"""
    o, res, dim = np.array(g["origin"]), g["res"], np.array(g["dim"])
    hi = o + dim * res
    pts = []
    for ax in range(3):
        for face in (o[ax], hi[ax]):
            for eps in (0.0, 1e-12, -1e-12, 1e-7, -1e-7, 0.49 * res, -0.49 * res):
                for _ in range(3):
                    p = rng.uniform(o, hi)
                    p[ax] = face + eps
                    pts.append(p)
        for k in list(range(-3, 4)) + [int(dim[ax]) - 1, int(dim[ax]), int(dim[ax]) + 1, int(dim[ax]) // 2]:
            p = rng.uniform(o, hi)
            p[ax] = o[ax] + k * res  # exactly on a face between cells
            pts.append(p)
            q = p.copy()
            q[(ax + 1) % 3] = o[(ax + 1) % 3] + float(rng.integers(0, dim[(ax + 1) % 3])) * res
            pts.append(q)
    pts += list(rng.uniform(o - 3 * res, hi + 3 * res, (300, 3)))
    pts += [-p for p in pts[:20]]  # (negative coordinates whatever the origin's sign)
    return np.array(pts)


def face_rays(g, rng):
    """rays from inside the map through each of the six faces, and random ones"""
    o, res, dim = np.array(g["origin"]), g["res"], np.array(g["dim"])
    hi = o + dim * res
    rays = []
    for ax in range(3):
        for sign in (-1, 1):
            for _ in range(3):
                a, b = rng.uniform(o, hi), rng.uniform(o, hi)
                b[ax] = (hi[ax] + rng.uniform(0.5, 4.0) * res) if sign > 0 else (o[ax] - rng.uniform(0.5, 4.0) * res)
                rays.append((a, b))
    rays += [(rng.uniform(o, hi), rng.uniform(o - 4 * res, hi + 4 * res)) for _ in range(12)]
    return rays


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_map_util_helpers_on_the_geometry(name):
    from mpl_ros_amd.planner import VoxelMapUtil
    small = name != LONG  # (the fine map has 1.8 M cells: fewer unknown cells, so the clouds stay small)
    grid, origin, res, start, goal, g = util.geometry(name, unknown=0.05 if small else 0.002)
    assert (grid == -1).sum() > 0 and (grid > 0).sum() > 0
    rng = np.random.default_rng(g["seed"])
    P = orc.Planner()
    P.set_map(grid, origin, res)
    mu = VoxelMapUtil()
    mu.setMap(origin, g["dim"], grid.ravel(), res)
    pts = face_points(g, rng)
    for value in (-1, 100):  # ... and the centres of some unknown and some occupied cells
        zyx = np.argwhere(grid == value)
        zyx = zyx[rng.choice(len(zyx), 20, replace=False)]
        pts = np.concatenate([pts, np.array(origin) + (zyx[:, ::-1] + 0.5) * res])
    # before any edit: cells and states of the points (floatToInt at the faces, negative coordinates)
    cells0, st0 = mu.query(pts)
    want = [P.float_to_int(p) for p in pts]
    assert [tuple(c) for c in cells0.tolist()] == want
    assert st0.tolist() == [P.cell_state(c) for c in want]
    assert {0, 1, 2, 3} <= set(st0.tolist())  # free, occupied, unknown, outside all occur
    assert any(min(c) < 0 for c in want) and any(c[ax] >= g["dim"][ax] for c in want for ax in range(3))
    dim = np.array(g["dim"])
    cells = np.concatenate([rng.integers(-3, dim + 3, size=(400, 3)), dim - 1 - rng.integers(0, 3, size=(60, 3)),
                            rng.integers(-1, 2, size=(30, 3))]).astype(np.int32)
    util.compare_map_helpers(P, mu, grid, cells, face_rays(g, rng), pts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_potential_and_search_region_on_the_geometry(name):
    """updatePotentialMap with and without a range, setSearchRegion around the oracle's path: the whole auxiliary map, and the
    counts of getSearchRegion / getPotentialCloud"""
    grid, origin, res, start, goal, g = util.geometry(name, unknown=0.02)
    U = util.geometry_lattice(g)
    kw = plan_kw(g, orc.ACC)
    radius = (4 * res, 4 * res, 3 * res)
    centre = util.geometry_point(g, (0.5, 0.5, 0.5))
    box = tuple(0.3 * g["dim"][i] * res for i in range(3))
    for range_ in (None, box):
        P = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
        P.set_potential_weights(3.0, 0)
        P.update_potential_map(radius, centre, range_ or (0, 0, 0))
        mu, pl = util.make_gpu(grid, origin, res, U, **kw)
        pl.setPotentialRadius(radius); pl.setPotentialWeight(3.0)
        if range_:
            pl.setPotentialMapRange(range_)
        pl.updatePotentialMap(centre)
        a = P.aux_map()
        assert ((a > 0) & (a < 100)).sum() > 50 and (a == 0).sum() > 50
        assert np.array_equal(util.aux_of(mu), a.ravel())
        assert len(pl.getPotentialCloud(1.0)) == int(((a > 0) & (a < 100)).sum())
    # the region around the first path, then the potential on top of it
    P = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
    assert P.plan(orc.waypoint(start), orc.waypoint(goal)) == orc.OK
    path = [tuple(w.pos) for w in P.traj()["wps"]]
    sr = (5 * res, 4 * res, 3 * res)
    P.set_search_region(path, sr)
    mu, pl = util.make_gpu(grid, origin, res, U, **kw)
    pl.setSearchRadius(sr); pl.setSearchRegion(path)
    reg = pl.getSearchRegion()
    a = P.aux_map()
    assert 0 < (a >= 0).sum() < a.size
    assert np.array_equal(util.aux_of(mu), a.ravel()) and len(reg) == int((a >= 0).sum())
    P.set_potential_weights(3.0, 0)
    P.update_potential_map(radius, start)
    pl.setPotentialRadius(radius); pl.setPotentialWeight(3.0)
    pl.updatePotentialMap(start)
    a = P.aux_map()
    assert np.array_equal(util.aux_of(mu), a.ravel())
    assert len(pl.getSearchRegion()) == int((a >= 0).sum()) and len(pl.getPotentialCloud(1.0)) == int(((a > 0) & (a < 100)).sum())


# ---------------------------------------------------------------------------------------------------------------- successors
def face_states(g, control, rng):
    """States whose primitives leave the map through each of the six faces: moving outwards at `speed`, at distances from the face
    that put the exit at sample 1, at a middle sample and at the last sample; the ones at the upper faces sit in the last (partial)
    brick of their axis.  Plus random interior states.  Returns (states, aimed face of each state or None)."""
    o, res, dim = np.array(g["origin"]), g["res"], np.array(g["dim"])
    hi = o + dim * res
    states, aimed = [], []
    zero = np.zeros(3)
    speed = 1.0 if control == orc.VEL else 1.5  # (a VEL primitive moves at its input, 1 m/s here, whatever the state)
    for ax in range(3):
        for sign in (-1, 1):
            for d in (0.3 * res, 0.5 * speed, speed - 0.4 * res, 0.25 * speed, 0.75 * speed, speed + 0.3 * res):
                for _ in range(4):
                    p = rng.uniform(o + 0.5 * res, hi - 0.5 * res)
                    p[ax] = (hi[ax] - d) if sign > 0 else (o[ax] + d)
                    if not (o[ax] < p[ax] < hi[ax]):
                        continue
                    v = np.zeros(3)
                    v[ax] = sign * speed
                    states.append((p, v, zero, zero))
                    aimed.append((ax, sign))
    for _ in range(60):
        p = rng.uniform(o + 0.5 * res, hi - 0.5 * res)
        v = np.round(rng.uniform(-2, 2, 3), 1)
        a = np.round(rng.uniform(-1, 1, 3), 1) if control & 4 else zero
        j = np.round(rng.uniform(-1, 1, 3), 1) if control & 8 else zero
        states.append((p, v, a, j))
        aimed.append(None)
    return states, aimed


def blocked_kinds(P, Pfree, states, info, control):
    """From the oracle alone: for every blocked successor whether it left the map (and at which sample) or met an occupied voxel.
    Pfree: the same geometry without obstacles -- a primitive blocked there leaves the map, at sample `reads`."""
    out = []  # (state index, kind, sample, n)
    for k, (p, v, a, j) in enumerate(states):
        cur = orc.waypoint(p, v, a, j, control, t=0.5 * k)
        acts = [ai for ai, _, _, _ in info[k]]
        free = util.succ_reads(Pfree, cur, P._U, acts)
        for (ai, co, reads, n), (r0, _) in zip(info[k], free):
            if not np.isinf(co):
                assert reads == n + 1  # a free primitive reads every sample
                continue
            if r0 < n + 1 and reads == r0:
                out.append((k, "left", r0, n))  # samples 0 .. r0 - 1 read, sample r0 outside
            else:
                out.append((k, "occupied", reads - 1, n))
    return out


SUCC_CASES = [(n, c) for n in NAMES for c in (orc.ACC, orc.JRK)] + [(n, c) for n in ("f32_005_mixed", "r025_thin", LONG) for c in (orc.SNP, orc.VEL)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", SUCC_CASES, ids=[f"{n}-{CN[c]}" for n, c in SUCC_CASES])
def test_successors_at_the_faces_of_the_geometry(name, control):
    grid, origin, res, start, goal, g = util.geometry(name, bubbles=False)
    U = mapgen.control_lattice(1.0, 1, True)  # 27 inputs on every geometry: the single-layer map is left upwards and downwards too
    kw = plan_kw(g, control, v_max=3.0)
    P = util.make_oracle(grid, origin, res, control, U, **kw)
    Pfree = util.make_oracle(np.zeros_like(grid), origin, res, control, U, **kw)
    rng = np.random.default_rng(100 + g["seed"] + control)
    states, aimed = face_states(g, control, rng)
    mu, pl = util.make_gpu(grid, origin, res, U, **kw)
    out = pl.getSuccBatch([util.gpu_wp(p, v, a, j, control, t=0.5 * i) for i, (p, v, a, j) in enumerate(states)])
    info = util.compare_succ(P, out, states, control, U, per_succ_reads=True)
    kinds = blocked_kinds(P, Pfree, states, info, control)
    left = [(k, s, n) for k, kind, s, n in kinds if kind == "left"]
    assert left and any(kind == "occupied" for _, kind, _, _ in kinds)  # both kinds of blocked successor
    assert any(s == 1 for _, s, _ in left) and any(1 < s < n for _, s, n in left) and any(s == n and n > 1 for _, s, n in left)
    for face in [(ax, sign) for ax in range(3) for sign in (-1, 1)]:  # every face is left by a state aimed at it
        assert any(aimed[k] == face for k, _, _ in left), face
    dim = g["dim"]
    last = [k for k, (p, _, _, _) in enumerate(states) for ax in range(3)
            if aimed[k] == (ax, 1) and P.float_to_int(p)[ax] >= 8 * ((dim[ax] - 1) // 8)]
    assert len({aimed[k] for k in last}) == 3  # states in the last brick of every axis


# ---------------------------------------------------------------------------------------------------------------- whole plans
def run_plan(name, control, U, spec=-1, helpers=None, kernel=None, max_expand=1500, start_vel=(0, 0, 0), yaw=None, yaw_max=-1.0, caps=None):
    grid, origin, res, start, goal, g = util.geometry(name)
    kw = plan_kw(g, control, max_expand=max_expand)
    if yaw is not None:
        kw["yaw_max"] = yaw_max
    P = util.make_oracle(grid, origin, res, control | (orc.YAW if yaw is not None else 0), U, **kw)
    mu, pl = util.make_gpu(grid, origin, res, U, spec=spec, **(caps or {}), **kw)
    out = []
    for h, kn in zip(helpers or [None], kernel if isinstance(kernel, (list, tuple)) else [kernel]):
        if h is not None:
            pl.setHelpers(*h)
        r, c = util.compare_plan(P, pl, start_of(control, start, start_vel), (goal,), control, yaw=yaw)
        assert pl.kernelName() == kn, pl.kernelName()
        assert r.n_expanded >= 100, r.n_expanded  # (the default-lattice ACC / JRK plans: >= 300, asserted by the CPU test above)
        out.append(r)
    return P, pl, out


# (SNP on the single-layer map is left out: with a_max = j_max = 1 the snap lattice runs out of valid primitives after 32 expansions)
ONE_NODE = [(n, c) for n in NAMES for c in (orc.ACC, orc.JRK, orc.SNP) if (n, c) != ("r015_flat", orc.SNP)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", ONE_NODE, ids=[f"{n}-{CN[c]}" for n, c in ONE_NODE])
def test_one_node_kernel_on_the_geometry(name, control):
    """setSpeculation(0): ACC, JRK and SNP states (SNP without yaw: no other voxel test plans it)"""
    g = util.GEOMETRIES[name]
    run_plan(name, control, util.geometry_lattice(g), spec=0, kernel=f"astar_kernel<64,{CN[control]}>")


WORD = ("status", "cost", "n_expanded", "expand_hash", "n_nodes", "n_edges", "n_closed", "voxel_reads", "n_succ", "n_succ_finite", "traj_len")
HELP_OFF, HELP_ON = (0, -1), (-1, -1)


def same_word(ra, rb):
    for k in WORD:
        assert getattr(ra, k) == getattr(rb, k), k


SPEC32 = [("f32_01_neg", True), ("f32_005_mixed", True), ("f32_005_mixed", False), ("r02_far", True), ("r025_thin", True), ("r015_flat", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("control", [orc.ACC, orc.JRK], ids=["ACC", "JRK"])
@pytest.mark.parametrize("name,use_3d", SPEC32, ids=[f"{n}-{27 if d else 9}" for n, d in SPEC32])
def test_speculative_32_lane_kernel_on_the_geometry(name, use_3d, control):
    """9- and 27-input lattices: 32 lanes x 16 units; without and with helper workgroups (the helper kernel samples too)"""
    g = util.GEOMETRIES[name]
    U = mapgen.control_lattice(g["u"], 1, use_3d)
    cn = CN[control]
    _, _, (r0, r1) = run_plan(name, control, U, helpers=[HELP_OFF, HELP_ON],
                              kernel=[f"astar_spec_kernel<32,16,{cn}>", f"astar_spec_kernel<32,16,{cn},help>"])
    same_word(r0, r1)


SPEC128 = ["f32_01_neg", "f32_005_mixed", "r02_far"]


@pytest.mark.gpu
@pytest.mark.parametrize("control", [orc.ACC, orc.JRK], ids=["ACC", "JRK"])
@pytest.mark.parametrize("name", SPEC128)
def test_speculative_128_lane_kernel_on_the_geometry(name, control):
    """125 inputs: 128 lanes x 4 units; the jerk build has a helper kernel, the acceleration build has none"""
    g = util.GEOMETRIES[name]
    U = mapgen.control_lattice(g["u"], 2, True)
    assert len(U) == 125
    cn = CN[control]
    on = f"astar_spec_kernel<128,4,{cn},help>" if control == orc.JRK else f"astar_spec_kernel<128,4,{cn}>"
    _, _, (r0, r1) = run_plan(name, control, U, helpers=[HELP_OFF, HELP_ON], kernel=[f"astar_spec_kernel<128,4,{cn}>", on], max_expand=600,
                              caps=dict(max_nodes=1 << 21, max_edges=1 << 23))
    same_word(r0, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32_01_neg", "f32_005_mixed", "r02_far", "r025_thin"])
def test_potential_builds_on_the_geometry(name):
    """potential plus search region on a 3-D map with dx != dy != dz: the `pot` build of the speculative kernel and of the one-node
    kernel"""
    grid, origin, res, start, goal, g = util.geometry(name)
    assert len(set(g["dim"])) == 3
    U = util.geometry_lattice(g)
    kw = plan_kw(g, orc.ACC)
    P = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
    assert P.plan(orc.waypoint(start), orc.waypoint(goal)) == orc.OK
    plain = P.traj_cost
    path = [tuple(w.pos) for w in P.traj()["wps"]]
    sr, radius = (1.2, 1.0, 0.8), (4 * res, 4 * res, 3 * res)
    P.set_search_region(path, sr)
    P.set_potential_weights(3.0, 0)
    P.update_potential_map(radius, start)
    mu, pl = util.make_gpu(grid, origin, res, U, **kw)
    pl.setSearchRadius(sr); pl.setSearchRegion(path)
    pl.setPotentialRadius(radius); pl.setPotentialWeight(3.0)
    pl.updatePotentialMap(start)
    a = P.aux_map()
    assert np.array_equal(util.aux_of(mu), a.ravel()) and (a < 0).sum() > 0 and ((a > 0) & (a < 100)).sum() > 100
    r, c = util.compare_plan(P, pl, (start, (0, 0, 0)), (goal,), orc.ACC)
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,pot>"
    assert r.status == 0 and r.cost >= plain and r.n_expanded >= 50
    pl.setSpeculation(0)
    r1, _ = util.compare_plan(P, pl, (start, (0, 0, 0)), (goal,), orc.ACC)
    assert pl.kernelName() == "astar_kernel<64,ACC>"
    same_word(r, r1)


YAW = [("f32_01_neg", "astar_spec_kernel<128,4,ACC,yaw>"), ("f32_005_mixed", "astar_spec_kernel<128,4,ACC,yaw>"),
       ("r015_flat", "astar_spec_kernel<32,16,ACC,yaw>"), (LONG, "astar_spec_kernel<32,16,ACC,yaw>")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", YAW, ids=[n for n, _ in YAW])
def test_yaw_builds_on_the_geometry(name, kernel):
    """yaw_max > 0 with the (x, y, z, yaw rate) lattices: 81 inputs in 3-D, 27 in the plane; then the one-node yaw kernel"""
    g = util.GEOMETRIES[name]
    U = mapgen.control_lattice(g["u"], 1, g["use_3d"], u_yaw=0.5)
    P, pl, (r,) = run_plan(name, orc.ACC, U, kernel=kernel, yaw=(0.4, 1.0), yaw_max=0.7, caps=dict(max_nodes=1 << 21, max_edges=1 << 23))
    grid, origin, res, start, goal, _ = util.geometry(name)
    pl.setSpeculation(0)
    r1, _ = util.compare_plan(P, pl, (start, (0, 0, 0)), (goal,), orc.ACC, yaw=(0.4, 1.0))
    assert pl.kernelName() == f"astar_kernel<{64 if len(U) <= 64 else 128},ACC,yaw>"
    same_word(r, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32_005_mixed", "f32_01_neg", "r025_thin"])
def test_plan_batch_on_the_geometry(name):
    """planBatch of several queries (more than slots) against the oracle's and the device's single queries"""
    grid, origin, res, start, goal, g = util.geometry(name)
    U = util.geometry_lattice(g)
    kw = plan_kw(g, orc.ACC, max_expand=3000)
    P = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
    queries = mapgen.random_queries(grid, origin, res, 10, mapgen.SplitMix64(g["seed"]), min_dist=0.45 * g["dim"][0] * res)
    mu, pl = util.make_gpu(grid, origin, res, U, n_slots=4, record=1 << 15, **kw)
    res_b = pl.planBatch([util.gpu_wp(s) for s, _ in queries], [util.gpu_wp(t) for _, t in queries])
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>"
    util.compare_plan_batch(P, pl, queries, res_b, 1 << 15)
    assert sum(r.n_expanded for r in res_b) >= 1000 and sum(r.status == 0 for r in res_b) >= 5
    words = [tuple(getattr(r, k) for k in WORD) for r in res_b]
    for q, (s, t) in enumerate(queries):
        pl.plan(util.gpu_wp(s), util.gpu_wp(t))
        assert tuple(getattr(pl.getResult(), k) for k in WORD) == words[q], q


# ---------------------------------------------------------------------------------------------------------------- LPA* and fleets
def corner_cells(P, dim):
    """free cells on and next to the upper faces: the 3^3 cube around (dx - 2, dy - 2, dz - 2), which lies in the last brick of every
    axis (cells beyond the faces are dropped by box_cells)"""
    o, res = P._origin_res
    centre = tuple(o[i] + (dim[i] - 1.5) * res for i in range(3))
    assert P.float_to_int(centre) == tuple(d - 2 for d in dim)
    return box_cells(P, centre, 1)


class GeoCase(Case):
    """A fleet scenario of test_lpa_fleet on a named geometry: members start -> goal, goal -> start and a third pair; the edit is the
    union of a box on the middle of every member's first path and the cells at the upper corner of the map."""

    def __init__(self, name, speed=0.0):
        self.name = "geo:" + name
        self.grid, self.origin, self.res, start, goal, g = util.geometry(name)
        self.g = g
        self.U = util.geometry_lattice(g)
        self.kw, self.control = plan_kw(g, orc.ACC), orc.ACC
        third = (util.geometry_point(g, (g["start"][0], g["goal"][1], g["start"][2])), util.geometry_point(g, (g["goal"][0], g["start"][1], g["goal"][2])))
        r = max(2, int(round(0.3 / self.res)))
        for p in third:
            mapgen.carve_bubble(self.grid, p, self.origin, self.res, r)
        self.pairs = [(start, goal), (goal, start), third]
        self.vel = [(speed, 0.0, 0.0), (-speed, 0.0, 0.0), (speed, 0.0, 0.0)]  # (every member sets out towards its goal)
        self.cap = (1 << 17, 1 << 20, 1 << 20)
        self.n = len(self.pairs)
        self.grid0 = self.grid.copy()
        self.scratch = util.make_oracle(self.grid, self.origin, self.res, self.control, self.U, **self.kw)
        self.L = [self.oracle(True) for _ in range(self.n)]

    def starts(self, g=False):
        return [(self.g_wp if g else self.o_wp)(s, v) for (s, _), v in zip(self.pairs, self.vel)]

    def block_cells(self):
        half = max(1, int(round(0.2 / self.res)))
        cells = set(corner_cells(self.scratch, self.g["dim"]))
        for L in self.L:
            tr = L.traj()
            cells |= set(box_cells(self.scratch, tuple(tr["wps"][tr["n"] // 2].pos), half))
        cells = sorted(cells)
        for x, y, z in cells:
            self.grid[z, y, x] = 100
        return cells


def lpa_scenario(name, speed=0.0, gpu=True):
    """plan, updateBlockedNodes (a box on the middle of the path and the cells at the upper corner), repair, updateClearedNodes, repair:
    the HIP LPA* against the oracle's after every step (compare_lpa).  gpu=False: the oracle side alone (the CPU test of the inputs).
    Returns the oracle planner."""
    from mpl_ros_amd.planner import VoxelMapPlanner
    grid, origin, res, start, goal, g = util.geometry(name)
    # the goal next to the upper corner: the repairs reach the last (partial) bricks
    goal = tuple(origin[i] + (g["dim"][i] - (6.5 if g["dim"][i] > 12 else 0.5 * g["dim"][i])) * res for i in range(3))
    mapgen.carve_bubble(grid, goal, origin, res, max(2, int(round(0.3 / res))))
    U = util.geometry_lattice(g)
    kw = plan_kw(g, orc.ACC)
    scratch = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
    L = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
    L.set_lpastar(True)
    if gpu:
        mu, a = util.make_gpu(grid, origin, res, U, **kw)
        l = VoxelMapPlanner(False)
        l.setMapUtil(mu)
        l.setVmax(kw["v_max"]); l.setAmax(kw["a_max"]); l.setDt(1.0); l.setU(U); l.setTol(kw["tol_pos"])
        l.setCapacity(1, 1 << 17, 1 << 20, 1 << 20)
        l.setLPAstar(True)
    vel = (speed, 0.0, 0.0)
    so, go, sg, gg = orc.waypoint(start, vel=vel), orc.waypoint(goal), util.gpu_wp(start, vel=vel), util.gpu_wp(goal)
    seen = []

    def replan():
        L.reset_counters()
        sl = L.plan(so, go)
        seen.append((sl, L.lpa_iterations()))
        if gpu:
            ok = l.plan(sg, gg)
            assert ok == (sl == orc.OK)
            compare_lpa(L, l, l.getResult(), sl)
            assert a.plan(sg, gg) == ok and (not ok or a.getResult().cost == l.getResult().cost)  # == a fresh device A*
        return sl

    def set_maps(m):
        scratch.set_map(m, origin, res)
        L.set_map(m, origin, res)
        if gpu:
            mu.setMap(origin, g["dim"], m.ravel(), res)

    assert replan() == orc.OK
    tr, cost0 = L.traj(), L.traj_cost
    corner = corner_cells(scratch, g["dim"])
    cells = sorted(set(corner) | set(box_cells(scratch, tuple(tr["wps"][tr["n"] // 2].pos), max(1, int(round(0.2 / res))))))
    dim = g["dim"]
    assert corner and any(c[ax] == dim[ax] - 1 for c in cells for ax in range(3)) and any(c[0] >= 8 * ((dim[0] - 1) // 8) for c in cells)
    g2 = grid.copy()
    for x, y, z in cells:
        g2[z, y, x] = 100
    set_maps(g2)
    nb = L.update_blocked(cells)
    assert nb > 0 and (not gpu or l.updateBlockedNodes(cells) == nb)
    replan()
    assert seen[-1][1] > 0  # the repair expands states
    set_maps(grid)
    nc = L.update_cleared(cells)
    assert nc > 0 and (not gpu or l.updateClearedNodes(cells) == nc)
    assert replan() == orc.OK and L.traj_cost == cost0
    return L


LPA_NAMES = ["f32_01_neg", "f32_005_mixed", "r025_thin"]
FLEET_NAMES = ["f32_01_neg", "f32_005_mixed", "r02_far"]  # (on the thin map the edit leaves two of the three members without a path)
LONG_SPEED = 2.6  # start speed on the fine map: the first primitives have n = 260 .. 310 samples


def test_oracle_lpa_and_fleet_inputs_on_the_geometries():
    """CPU: the LPA* scenarios and the fleet cases are what the GPU tests need (paths exist, edits touch the state space)"""
    for name in LPA_NAMES + [SPARSE]:
        lpa_scenario(name, LONG_SPEED if name == SPARSE else 0.0, gpu=False)
    for name in FLEET_NAMES + [SPARSE]:
        speed = LONG_SPEED if name == SPARSE else 0.0
        case = GeoCase(name, speed)
        touched = []

        def check(label, res, counts):
            if counts is not None:
                touched.append(sum(counts[0]))
            elif label == "first":
                assert all(s == orc.OK for s in res[0].values()), (name, label, res[0])
                assert name != SPARSE or all(long_regimes(L, case.U, 2048)[0] for L in case.L)  # n > 255 in every member's first plan
            elif label == "blocked":  # (a robot at 2.6 m/s may find no way round the new box: NO_PATH is compared like any status)
                assert any(s == orc.OK for s in res[0].values()), (name, label, res[0])
            else:
                assert all(s == orc.OK for s in res[0].values()), (name, label, res[0])  # every member has a path

        replay(case, [CheckerSide(case)], None, check, True)
        assert len(touched) == 2 and min(touched) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", LPA_NAMES)
def test_lpastar_on_the_geometry(name):
    lpa_scenario(name)


def fleet_scenario(name, speed=0.0, probe=None):
    """probe(L): called for every member's checker after the first plan (oracle-side regime checks); the results are returned"""
    case = GeoCase(name, speed)
    probed = []
    mu, _ = case.gpu()
    fleet = case.fleet(mu)
    fs = FleetSide(case, fleet)
    seen = []

    def check(label, res, counts):
        seen.append(label)
        if counts is not None:
            assert counts[1] == counts[0]  # per member, the checker's
            return
        st_o, rg = res
        if label == "first" and probe:
            probed.extend(probe(L) for L in case.L)
        check_fleet(case, fleet, rg, st_o)
        assert fs.stats[-1] == ([0, 0, case.n, 0] if label == "first" else [case.n, 1, 0, 0])

    replay(case, [CheckerSide(case), fs], mu, check, True)
    assert seen == ["first", "block", "blocked", "clear", "cleared", "moved on"] and case.n >= 3
    return probed


@pytest.mark.gpu
@pytest.mark.parametrize("name", FLEET_NAMES)
def test_lpa_fleet_on_the_geometry(name):
    fleet_scenario(name)


@pytest.mark.gpu
def test_voxel_grid_with_a_negative_origin_hands_its_map_to_the_planner():
    """VoxelGrid at origin (-3, -2, 0) (119 x 89 x 29 cells), setMapUtil device to device, then a plan against the oracle on
    orc.Grid's map"""
    from mpl_ros_amd.planner import VoxelMapPlanner, VoxelMapUtil
    from mpl_ros_amd.voxel_grid import VoxelGrid
    rng = np.random.default_rng(3)
    origin, dim, res = (-3.0, -2.0, 0.0), (12.0, 9.0, 3.0), 0.1
    G, O = VoxelGrid(origin, dim, res), orc.Grid(origin, dim, res)
    pts = rng.uniform((-2.0, -1.0, 0.0), (8.0, 6.0, 3.0), (2500, 3))
    start, goal = (-2.45, -1.45, 1.55), (8.45, 6.45, 1.55)
    pts = pts[(np.linalg.norm(pts[:, :2] - start[:2], axis=1) > 0.8) & (np.linalg.norm(pts[:, :2] - goal[:2], axis=1) > 0.8)]
    ns = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (0, 1)]
    a, b = G.addCloud(pts, ns), O.add_cloud(pts, ns)
    assert np.array_equal(a, b)
    U = mapgen.control_lattice(1.0, 1, True)
    mu, pl = VoxelMapUtil(), VoxelMapPlanner(False)
    G.setMapUtil(mu)
    assert np.array_equal(mu.getMap(), O.get_map())
    gdim, gori, gres = O.info()
    assert gdim == (119, 89, 29) and gori == origin  # (res is float32(0.1): 12 m hold 119 cells) -- dx != dy != dz, partial bricks
    grid = O.get_map().reshape(gdim[2], gdim[1], gdim[0])
    P = util.make_oracle(grid, gori, float(gres), orc.ACC, U, v_max=2.0, a_max=1.0)
    pl.setMapUtil(mu)
    pl.setVmax(2.0); pl.setAmax(1.0); pl.setDt(1.0); pl.setU(U); pl.setTol(0.5)
    pl.setCapacity(1, 1 << 20, 1 << 22, 1 << 21)
    r, c = util.compare_plan(P, pl, (start, (0, 0, 0)), (goal,), orc.ACC)
    assert r.status == 0 and r.n_expanded >= 200 and pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>"


# ---------------------------------------------------------------------------------------------------------------- long primitives
# res = 0.01: n = ceil(max_v dt / res) goes past 255, where the staged sampling path (8-bit sample index, owner map of 576 / 1536 /
# 2048 entries) hands over to the generic loop.  All regime checks come from the oracle (util.succ_reads, util.expanded_samples).
def long_states(rng, g, control):
    o, res, dim = np.array(g["origin"]), g["res"], np.array(g["dim"])
    hi = o + dim * res
    zero = np.zeros(3)
    out = []
    for vx in (2.535, 2.545, 2.555, 2.565, 3.0, 3.2, 2.0, 2.1, 2.101, 2.11, 2.15, 2.19, 2.195, 2.2, 1.0, 0.3, 0.0):
        for sign in (1, -1):
            for _ in range(3):
                p = rng.uniform(o + 0.5 * res, hi - 0.5 * res)
                p[2] = o[2] + 3.5 * res
                v = np.array([sign * vx, round(float(rng.uniform(-0.3, 0.3)), 1), 0.0])
                if rng.integers(0, 2):
                    v = v[[1, 0, 2]]  # ... and the same speeds along y
                out.append((p, v, zero, zero))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("control", [orc.ACC, orc.JRK], ids=["ACC", "JRK"])
@pytest.mark.parametrize("n_inputs", [3, 9])
def test_long_primitives_successors_r001_sparse(n_inputs, control):
    """Successor level.  3 inputs: a node's samples always fit the owner map, so a primitive's own n (254 .. 257) decides the path;
    9 inputs: the node's summed samples fall on both sides of 2048."""
    grid, origin, res, start, goal, g = util.geometry(SPARSE, bubbles=False)  # (few obstacles: some 2.5 m primitives are free)
    U = mapgen.control_lattice(g["u"], 1, False)
    if n_inputs == 3:
        U = U[[4, 1, 5]]  # (0, 0), (-u, 0), (0, +u): max_v is the state's own speed
        assert U[0].tolist() == [0, 0, 0] and U[1].tolist() == [-g["u"], 0, 0] and U[2].tolist() == [0, g["u"], 0]
    kw = plan_kw(g, control)
    P = util.make_oracle(grid, origin, res, control, U, **kw)
    states = long_states(np.random.default_rng(7 + control), g, control)
    # the regimes, from the oracle alone
    ns = [util.node_samples(P, orc.waypoint(p, v, a, j, control), U) for p, v, a, j in states]
    flat = {n for row in ns for n in row}
    assert {254, 255, 256, 257} <= flat and max(flat) >= 300 and min(flat) <= 50
    if n_inputs == 3:
        assert any(max(row) == 255 and sum(row) <= 2048 for row in ns if row) and any(max(row) == 256 and sum(row) <= 2048 for row in ns if row)
    else:
        sums = [sum(row) for row in ns if row]
        assert any(2000 < s <= 2048 for s in sums) and any(2048 < s < 2100 for s in sums) and any(s < 1000 for s in sums) and any(s > 2500 for s in sums)
    mu, pl = util.make_gpu(grid, origin, res, U, **kw)
    out = pl.getSuccBatch([util.gpu_wp(p, v, a, j, control, t=0.5 * i) for i, (p, v, a, j) in enumerate(states)])
    info = util.compare_succ(P, out, states, control, U, per_succ_reads=True)
    free_n = {n for row in info for _, co, reads, n in row if not np.isinf(co) and reads == n + 1}
    assert {254, 255, 256, 257} & free_n and max(free_n) >= 300  # unblocked primitives on both sides of the hand-over


def long_regimes(P, U, owner):
    """(an expanded node has a primitive with n > 255, one has summed samples <= owner, one has more) of the oracle's last plan"""
    ns = [row for row in util.expanded_samples(P, U) if row]
    return any(max(r) > 255 for r in ns), any(sum(r) <= owner for r in ns), any(sum(r) > owner for r in ns)


LONG_PLANS = [("one_node", 0, 0.5, 1, False, 2048, "astar_kernel<64,ACC>", "astar_kernel<64,ACC>"),
              ("spec32", -1, 0.5, 1, False, 576, "astar_spec_kernel<32,16,ACC>", "astar_spec_kernel<32,16,ACC,help>"),
              ("spec128", -1, 0.1, 2, True, 1536, "astar_spec_kernel<128,4,ACC>", "astar_spec_kernel<128,4,ACC>")]


@pytest.mark.gpu
@pytest.mark.parametrize("label,spec,u,num,use_3d,owner,k_off,k_on", LONG_PLANS, ids=[c[0] for c in LONG_PLANS])
def test_long_primitives_plans_r001_sparse(label, spec, u, num, use_3d, owner, k_off, k_on):
    """Plan level: a start from rest and a start at 2.6 m/s through each kernel family; the oracle's expansions show a primitive with
    n > 255 and summed samples on both sides of the family's owner map"""
    grid, origin, res, start, goal, g = util.geometry(SPARSE)
    U = mapgen.control_lattice(u, num, use_3d)
    kw = plan_kw(g, orc.ACC, max_expand=600)
    P = util.make_oracle(grid, origin, res, orc.ACC, U, **kw)
    mu, pl = util.make_gpu(grid, origin, res, U, spec=spec, max_nodes=1 << 21, max_edges=1 << 23, **kw)
    seen = np.zeros(3, dtype=bool)
    for vel in ((0, 0, 0), (LONG_SPEED, 0, 0)):
        words = []
        for h, kn in ((HELP_OFF, k_off), (HELP_ON, k_on)):
            pl.setHelpers(*h)
            r, c = util.compare_plan(P, pl, (start, vel), (goal,), orc.ACC)
            assert pl.kernelName() == kn and r.n_expanded >= 30  # (a robot at 2.6 m/s on a 10 m map: short searches)
            words.append(r)
        same_word(*words)
        seen |= np.array(long_regimes(P, U, owner))
    assert seen.all(), seen


@pytest.mark.gpu
def test_long_primitives_lpastar_r001_sparse():
    L = lpa_scenario(SPARSE, LONG_SPEED)
    assert long_regimes(L, L._U, 2048)[0]


@pytest.mark.gpu
def test_long_primitives_lpa_fleet_r001_sparse():
    U = util.geometry_lattice(util.GEOMETRIES[SPARSE])
    probed = fleet_scenario(SPARSE, LONG_SPEED, probe=lambda L: long_regimes(L, U, 2048)[0])
    assert len(probed) == 3 and all(probed)  # every member's first plan expands nodes with a primitive of n > 255
