"""The device-resident VoxelGrid (mplx_grid_*, mpl_ros_amd/csrc/mplx_grid.inl) swept over geometries, edges and operation
orders: tests/grid_scenes.py gives named grids (unaligned and far origins, odd resolutions, flat, 1-cell axes, column counts
around the scan's 1024-wide chunk, more cells / columns than the 4096 x 256 grid-stride launches have threads), clouds aimed
at the cell faces, and operation sequences with every form of `allocate` and of `addCloud(pts, ns)`.

CPU half: the oracle's restatement (orc.Grid) equals the compiled reference (oracle/_ref) after every operation, and every
scene shows the regime it is there for.  GPU half: the device grid equals the oracle (and the compiled reference, where it is
built) bit for bit after every operation -- both maps, getCloud (order and f64 bit patterns), new_obs with its order, the
allocate flag, info().  All comparisons are exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import orc
from tests import grid_scenes as gs
from tests.grid_scenes import SCENES, RefGrid

HAVE_REF = os.path.exists(RefGrid.PATH)
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built (needs /root/reference: make -C oracle ref)")


# ---------------------------------------------------------------------------------------------------------------- CPU half
def test_scene_table_gives_the_intended_cell_counts():
    """dim / res_float truncates: the table's counts must be the ones that actually come out"""
    for name, sc in SCENES.items():
        dim, ori, res = orc.Grid(sc["origin"], sc["size"], sc["res"]).info()
        assert dim == sc["cells"], (name, dim)
        assert ori == sc["origin"] and res == np.float32(sc["res"])
        assert gs.cells_of(sc["size"], sc["origin"], sc["res"])[0] == dim
    c = {n: SCENES[n]["cells"] for n in SCENES}
    assert [c[n][0] * c[n][1] for n in ("scan_1023", "scan_1024", "scan_1025")] == [1023, 1024, 1025]
    assert c["flat"][2] == 1 and SCENES["flat"]["size"][2] == 0.0 and SCENES["flat"]["origin"][2] == 0.0
    assert c["line_x"][1:] == (1, 1) and c["line_x"][0] > 1 and c["one_cell"] == (1, 1, 1)
    stride = 4096 * 256
    assert int(np.prod(c["cells_over_stride"])) > stride and c["cells_over_stride"][0] * c["cells_over_stride"][1] < stride
    assert c["cols_over_stride"][0] * c["cols_over_stride"][1] > stride
    assert any(abs(o / gs.f32(0.1) - round(o / gs.f32(0.1))) > 0.05 for o in SCENES["neg_unaligned"]["origin"])
    # the refusal: z size 0 off z origin 0 leaves no layer
    assert gs.cells_of(gs.FLAT_OFF["size"], gs.FLAT_OFF["origin"], gs.FLAT_OFF["res"])[0][2] == 0


def test_sequences_hold_every_operation_form():
    for name, sc in SCENES.items():
        ops = gs.sequence(name)
        kinds = [op[0] for op in ops]
        assert len(ops) <= 13 if sc["large"] else 35 <= len(ops) <= 45, (name, len(ops))
        # an addCloud(pts, ns) after an allocate, and one after a decay
        assert any(k == "add_ns" and "allocate" in kinds[:i] for i, k in enumerate(kinds)), name
        assert any(k == "add_ns" and "decay" in kinds[:i] for i, k in enumerate(kinds)), name
        if not sc["large"]:
            forms = {op[3] for op in ops if op[0] == "allocate"}
            assert forms >= {"same", "grow", "shrink", "shift_up", "shift_down", "disjoint", "origin_only", "size_only", "home"}, (name, forms)
            assert forms & {"flat", "thick"}
            assert {op[3] for op in ops if op[0] == "add_ns"} == set(gs.NS_SETS)
            assert {len(op) for op in ops if op[0] == "fill"} == {3, 4} and {len(op) for op in ops if op[0] == "clear"} == {1, 3}
            assert {op[1] for op in ops if op[0] == "decay"} == {1, 2, 3}
    assert (0, 0, 0) not in gs.NS_RING3 and len(set(gs.NS_DUP)) < len(gs.NS_DUP) and max(max(abs(v) for v in o) for o in gs.NS_RING3) == 3


# What the oracle counts on each scene's sequence (fixed seeds): points truncated into cell 0 from below the origin, (inside
# point, offset) pairs clipped at a face, cells hit by several points of one call, allocates that carried over nothing /
# something, new_obs cells that had decayed and flipped again, out-of-range fills.
COUNTS = {
    "neg_unaligned": (180, 16541, 1075, 1, 9, 6560, 2),
    "pos_far": (172, 15521, 1081, 3, 7, 5510, 2),
    "r025_exact": (188, 18204, 1093, 2, 6, 4455, 2),
    "r03": (179, 24995, 1292, 1, 8, 2784, 2),
    "third": (178, 25699, 1334, 1, 9, 2705, 2),
    "flat": (180, 25056, 818, 2, 8, 1253, 2),
    "line_x": (182, 7895, 151, 4, 5, 87, 2),
    "one_cell": (156, 10312, 102, 4, 6, 63, 2),
    "scan_1023": (180, 31686, 1242, 2, 7, 2777, 2),
    "scan_1024": (174, 35502, 1307, 2, 8, 2526, 2),
    "scan_1025": (180, 30313, 1133, 2, 7, 2733, 2),
    "cells_over_stride": (63, 15713, 2792, 1, 1, 2306, 1),
    "cols_over_stride": (66, 174600, 6628, 1, 1, 477, 1),
}


def regime_counts(name):
    sc = SCENES[name]
    O = orc.Grid(sc["origin"], sc["size"], sc["res"])
    n = {"below": 0, "clipped": 0, "multi": 0, "carry_none": 0, "carry_some": 0, "reflip": 0, "fill_out": 0}
    for op in gs.sequence(name):
        dim, ori, res = O.info()
        dim_a = np.array(dim)
        occ_before = int((O.get_map() > 0).sum())
        infl_before = O.get_map(True).reshape(dim[2], dim[1], dim[0])
        if op[0] in ("add", "add_ns"):
            with np.errstate(invalid="ignore", over="ignore"):
                q = (op[1] - np.array(ori)) / float(res)
                cell = np.trunc(q)
                inside = np.all(np.isfinite(q) & (cell >= 0) & (cell < dim_a), axis=1)
                n["below"] += int((inside & np.any((q < 0) & (q > -1), axis=1)).sum())
            cin = cell[inside].astype(np.int64)
            _, hits = np.unique(cin, axis=0, return_counts=True)
            n["multi"] += int((hits > 1).sum())
            if op[0] == "add_ns" and len(op[2]):
                nb = cin[:, None, :] + np.array(op[2])[None, :, :]
                n["clipped"] += int(np.any((nb < 0) | (nb >= dim_a), axis=2).sum())
        if op[0] == "fill" and not (0 <= op[1] < dim[0] and 0 <= op[2] < dim[1] and (len(op) == 3 or 0 <= op[3] < dim[2])):
            n["fill_out"] += 1
        if op[0] == "clear" and len(op) == 3:
            assert 0 <= op[1] < dim[0] and 0 <= op[2] < dim[1]  # the reference's clear(nx, ny) has no bounds test
        r = gs.apply(O, op)
        if op[0] == "add_ns":
            n["reflip"] += int(sum(infl_before[z, y, x] > 0 for x, y, z in r))
        if op[0] == "allocate":
            assert (O.info()[1], O.info()[0]) == op[4], (name, op[3])  # the generator's own bookkeeping of the geometry
            if r and occ_before > 0:
                n["carry_some" if (O.get_map() > 0).any() else "carry_none"] += 1
    return tuple(n.values())


def test_every_scene_shows_what_it_is_for():
    got = {name: regime_counts(name) for name in SCENES}
    print(json.dumps(got))
    for name, (below, clipped, multi, carry_none, carry_some, reflip, fill_out) in got.items():
        assert below > 0 and clipped > 0 and multi > 0 and carry_none > 0 and carry_some > 0 and reflip > 0 and fill_out > 0, (name, got[name])
    assert got == COUNTS


@needs_ref
@pytest.mark.parametrize("name", list(SCENES))
def test_restatement_matches_the_compiled_reference_on_the_scene(name):
    gs.run_lockstep(name, [orc.Grid, RefGrid])


def nonfinite_cloud(rng, sc):
    """good points with NaN / inf / 1e300 ones among them: all three coordinates, and one at a time with the other two inside"""
    o, nd, r = np.array(sc["origin"]), np.array(sc["cells"], dtype=np.float64), gs.f32(sc["res"])
    good = o + rng.uniform(0.1, 0.9, (60, 3)) * nd * r
    bad = []
    for v in (np.nan, np.inf, -np.inf, 1e300, -1e300):
        bad.append(np.array([v, v, v]))
        for axis in range(3):
            p = o + rng.uniform(0.1, 0.9, 3) * nd * r
            p[axis] = v
            bad.append(p)
    bad = np.array(bad)
    pts = np.concatenate([good[:30], bad, good[30:]])
    rng.shuffle(pts)
    return pts, bad


SINGLE_POINT_SCENES = ["neg_unaligned", "flat", "one_cell"]


def run_single_points(name, grids):
    """n == 1 in both addCloud forms: a point inside, the same point again (its cell is occupied: nothing inflates), a point
    outside, a point in the corner cell (offsets clipped at three faces), and the first point once more after a decay"""
    sc = SCENES[name]
    o, nd, r = np.array(sc["origin"]), np.array(sc["cells"], dtype=np.float64), gs.f32(sc["res"])
    p_in = (o + (np.floor(nd / 2) + 0.4) * r).reshape(1, 3)
    p_in2 = (o + (np.floor(nd / 3) + 0.6) * r).reshape(1, 3)
    p_corner = (o + (nd - 0.5) * r).reshape(1, 3)
    p_out = (o + (nd + 0.5) * r).reshape(1, 3)
    p_below = (o - 1.5 * r).reshape(1, 3)
    ops = [("add_ns", p_in, gs.NS_18, "18"), ("add_ns", p_in, gs.NS_18, "18"), ("add_ns", p_out, gs.NS_18, "18"), ("add", p_below),
           ("add", p_in2), ("add_ns", p_in2, gs.NS_RING3, "ring3"), ("add_ns", p_corner, gs.NS_RING3, "ring3"), ("add", p_corner),
           ("add_ns", p_below, gs.NS_DUP, "dup"), ("decay", 1), ("add_ns", p_in, gs.NS_DUP, "dup"), ("add_ns", p_in, gs.NS_SETS["empty"], "empty"),
           ("add_ns", p_corner, gs.NS_SETS["centre"], "centre"), ("clear",), ("add_ns", p_corner, gs.NS_18, "18"), ("add", p_out)]
    G = [make(sc["origin"], sc["size"], sc["res"]) for make in grids]
    news = []
    for i, op in enumerate(ops):
        res = [gs.apply(g, op) for g in G]
        ref = gs.state(G[0])
        for rr, g in zip(res[1:], G[1:]):
            gs.assert_same_result(res[0], rr, (name, i, op[0]))
            gs.assert_same_state(ref, gs.state(g), (name, i, op[0]))
        news.append(None if res[0] is None else len(res[0]))
    # from the oracle: the first call inflates, the repeat and the outside points do not, the decayed cell flips again
    assert news[0] > 0 and news[1] == 0 and news[2] == 0 and news[8] == 0 and news[10] > 0 and news[11] == 0 and news[14] > 0
    return news


@needs_ref
@pytest.mark.parametrize("name", SINGLE_POINT_SCENES)
def test_restatement_matches_the_compiled_reference_on_one_point_clouds(name):
    run_single_points(name, [orc.Grid, RefGrid])


NONFINITE_SCENES = ["neg_unaligned", "pos_far", "flat", "one_cell"]


def run_nonfinite(name, grids):
    sc = SCENES[name]
    rng = np.random.default_rng(77)
    pts, bad = nonfinite_cloud(rng, sc)
    G = [make(sc["origin"], sc["size"], sc["res"]) for make in grids]
    for i, op in enumerate([("add", bad), ("add_ns", bad, gs.NS_18, "18"), ("add", pts), ("decay", 1), ("add_ns", pts, gs.NS_18, "18"),
                            ("clear",), ("add_ns", pts, gs.NS_RING3, "ring3"), ("add_ns", bad, gs.NS_DUP, "dup")]):
        res = [gs.apply(g, op) for g in G]
        ref = gs.state(G[0])
        if i < 2:  # nothing but non-finite points so far: nothing is marked, nothing is reported
            assert not ref[1].any() and not ref[2].any() and len(ref[3]) == 0 and (res[0] is None or len(res[0]) == 0)
        for r, g in zip(res[1:], G[1:]):
            gs.assert_same_result(res[0], r, (name, i, op[0]))
            gs.assert_same_state(ref, gs.state(g), (name, i, op[0]))


@pytest.mark.parametrize("name", NONFINITE_SCENES)
def test_oracle_skips_non_finite_points(name):
    """NaN is a depth sensor's "no return": the reference's x86 convert makes it INT_MIN, a point outside"""
    run_nonfinite(name, [orc.Grid])


@needs_ref
@pytest.mark.parametrize("name", NONFINITE_SCENES)
def test_restatement_matches_the_compiled_reference_on_non_finite_points(name):
    run_nonfinite(name, [orc.Grid, RefGrid])


# ---------------------------------------------------------------------------------------------------------------- GPU half
def device_grid(origin, size, res):
    from mpl_ros_amd.voxel_grid import VoxelGrid
    return VoxelGrid(origin, size, res)


def parties():
    return [orc.Grid, device_grid] + ([RefGrid] if HAVE_REF else [])


def map_clouds_match(mu, O):
    """VoxelMapUtil's occupied and free clouds on the grid's map (the scan kernels through their other caller)"""
    dim, ori, res = O.info()
    P = orc.Planner()
    P.set_map(O.get_map().reshape(dim[2], dim[1], dim[0]), ori, float(res))
    occ, free = mu.getCloud(), mu.getFreeCloud()
    assert len(occ) + len(free) == dim[0] * dim[1] * dim[2] and len(occ) > 0
    for got, want in ((occ, P.cloud(0)), (free, P.cloud(1))):
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(occ.view(np.uint64), O.get_cloud().view(np.uint64))


def back_home(O, G, sc, seed):
    """both grids back on the scene's first geometry, emptied, with one fresh inflated cloud"""
    for g in (O, G):
        g.allocate(sc["size"], sc["origin"])
        g.clear()
    assert O.info()[0] == sc["cells"] and O.info()[1] == sc["origin"]
    pts = gs.make_points(np.random.default_rng(seed), sc["origin"], sc["cells"], sc["res"], 40)
    a, b = O.add_cloud(pts, gs.NS_18), G.addCloud(pts, gs.NS_18)
    assert np.array_equal(a, b) and len(a) > 0
    gs.assert_same_state(gs.state(O), gs.state(G), "back home")


def plan_through_the_inflated_map(O, G, sc):
    """a fresh cloud inflated by its neighbourhood, getInflatedMap() handed to the planner device to device, one plan"""
    from mpl_ros_amd import mapgen
    from mpl_ros_amd.planner import VoxelMapPlanner, VoxelMapUtil
    from tests import util
    rng = np.random.default_rng(5)
    for g in (O, G):
        g.allocate(sc["size"], sc["origin"])
        g.clear()
    dim, ori, res = O.info()
    assert dim == sc["cells"] and ori == sc["origin"]
    o, ext = np.array(ori), np.array(dim) * float(res)
    start, goal = o + (0.75, 0.75, 1.05), o + ext - (0.75, 0.75, 1.05)
    pts = o + rng.uniform(0.0, 1.0, (40, 3)) * ext
    pts = pts[(np.linalg.norm(pts[:, :2] - start[:2], axis=1) > 1.2) & (np.linalg.norm(pts[:, :2] - goal[:2], axis=1) > 1.2)]
    a, b = O.add_cloud(pts, gs.NS_18), G.addCloud(pts, gs.NS_18)
    assert np.array_equal(a, b) and len(a) > len(pts)
    U = mapgen.control_lattice(1.0, 1, True)
    mu, pl = VoxelMapUtil(), VoxelMapPlanner(False)
    G.setMapUtil(mu, inflated=True)
    assert np.array_equal(mu.getMap(), O.get_map(True)) and not np.array_equal(O.get_map(True), O.get_map())
    P = util.make_oracle(O.get_map(True).reshape(dim[2], dim[1], dim[0]), ori, float(res), orc.ACC, U, v_max=2.0, a_max=1.0)
    pl.setMapUtil(mu)
    pl.setVmax(2.0); pl.setAmax(1.0); pl.setDt(1.0); pl.setU(U); pl.setTol(0.5)
    pl.setCapacity(1, 1 << 20, 1 << 22, 1 << 21)
    r, c = util.compare_plan(P, pl, (tuple(start), (0, 0, 0)), (tuple(goal),), orc.ACC)
    assert r.status == 0 and r.n_expanded >= 5


def hundred_decays(O, G, sc):
    """an occupied cell reads 100 through the 99th decay and 0 after the 100th"""
    back_home(O, G, sc, 9)
    first = gs.state(O)
    assert first[1].max() == 100 and first[2].max() == 100
    for k in range(1, 101):
        O.decay(); G.decay()
        s = gs.state(G)
        gs.assert_same_state(gs.state(O), s, ("decay", k))
        if k < 100:
            assert np.array_equal(s[1], first[1]) and np.array_equal(s[2], first[2])
        else:
            assert not s[1].any() and not s[2].any() and len(s[3]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_device_grid_on_the_scene(name):
    from mpl_ros_amd.planner import VoxelMapUtil
    sc = SCENES[name]
    grids = gs.run_lockstep(name, parties())
    O, G = grids[0], grids[1]
    # clear(nx, ny) out of range, on the device alone (the reference's has no bounds test): nothing changes
    dim = O.info()[0]
    before = gs.state(G)
    for nx, ny in [(-1, 0), (0, -1), (dim[0], 0), (0, dim[1]), (dim[0] + 7, dim[1] + 7)]:
        G.clear(nx, ny)
    gs.assert_same_state(before, gs.state(G), (name, "clear out of range"))
    gs.assert_same_state(gs.state(O), before, (name, "end"))
    # getMap() / getInflatedMap() into a MapUtil, device to device
    mu = VoxelMapUtil()
    G.setMapUtil(mu)
    assert tuple(int(v) for v in mu.getDim()) == dim and tuple(mu.getOrigin()) == O.info()[1] and mu.getRes() == float(O.info()[2])
    assert np.array_equal(mu.getMap(), O.get_map()) and O.get_map().any()
    if name in ("cols_over_stride", "scan_1025"):
        map_clouds_match(mu, O)
    G.setMapUtil(mu, inflated=True)
    assert np.array_equal(mu.getMap(), O.get_map(True)) and not np.array_equal(O.get_map(True), O.get_map())
    if name == "scan_1025":  # ... and on the table's own 1025 columns (the sequence ends on a grown grid)
        back_home(O, G, sc, 7)
        G.setMapUtil(mu)
        assert tuple(int(v) for v in mu.getDim()) == sc["cells"]
        map_clouds_match(mu, O)
    if name == "r03":
        plan_through_the_inflated_map(O, G, sc)
    if name in ("line_x", "one_cell"):
        hundred_decays(O, G, sc)


@pytest.mark.gpu
def test_device_refuses_a_grid_without_a_layer():
    """flat_off: z size 0 at z origin 0.5 gives nd[2] = 0"""
    from mpl_ros_amd import _capi
    from mpl_ros_amd.voxel_grid import VoxelGrid
    f = gs.FLAT_OFF
    with pytest.raises(_capi.MplxError, match="empty grid"):
        VoxelGrid(f["origin"], f["size"], f["res"])
    sc = SCENES["flat"]
    G, O = VoxelGrid(sc["origin"], sc["size"], sc["res"]), orc.Grid(sc["origin"], sc["size"], sc["res"])
    pts = gs.make_points(np.random.default_rng(2), sc["origin"], sc["cells"], sc["res"], 50)
    assert np.array_equal(G.addCloud(pts, gs.NS_18), O.add_cloud(pts, gs.NS_18))
    with pytest.raises(_capi.MplxError, match="empty grid"):
        G.allocate(f["size"], f["origin"])
    gs.assert_same_state(gs.state(O), gs.state(G), "a refused allocate leaves the grid as it was")
    assert np.array_equal(G.addCloud(pts[::-1], gs.NS_RING3), O.add_cloud(pts[::-1], gs.NS_RING3))
    gs.assert_same_state(gs.state(O), gs.state(G), "after the refusal")


@pytest.mark.gpu
def test_c_call_edges_of_the_grid():
    """mplx_grid_add_cloud_inflate with cap below n_new, mplx_grid_get_cloud with cap below the total, n == 0, n_ns == 0"""
    from mpl_ros_amd.voxel_grid import VoxelGrid
    sc = SCENES["neg_unaligned"]
    mk = lambda: VoxelGrid(sc["origin"], sc["size"], sc["res"])  # noqa: E731
    A, B, O = mk(), mk(), orc.Grid(sc["origin"], sc["size"], sc["res"])
    lib = A.lib
    pts = gs.make_points(np.random.default_rng(11), sc["origin"], sc["cells"], sc["res"], 200)
    ns = np.array(gs.NS_18, dtype=np.int32)

    def inflate(G, p, o, cap):
        out = np.full((max(cap, 1), 3), -77, dtype=np.int32)
        n = C.c_int(-1)
        G._check(lib.mplx_grid_add_cloud_inflate(G.h, p.shape[0], p.ctypes.data if p.size else None, o.shape[0], o.ctypes.data if o.size else None,
                                                  out.ctypes.data if cap else None, cap, C.byref(n)))
        return n.value, out

    full = A.addCloud(pts, ns)
    want = O.add_cloud(pts, ns)
    assert np.array_equal(full, want) and len(full) > 40
    cap = len(full) // 3
    n_new, head = inflate(B, pts, ns, cap)
    assert n_new == len(full) and np.array_equal(head[:cap], full[:cap])
    gs.assert_same_state(gs.state(A), gs.state(B), "capped new_obs")
    gs.assert_same_state(gs.state(O), gs.state(B), "capped new_obs")
    # cap 0 with no buffer at all, on the decayed grid
    for g in (A, B, O):
        g.decay()
    full = A.addCloud(pts[::-1], ns)
    assert np.array_equal(full, O.add_cloud(pts[::-1], ns)) and len(full) > 40
    n_new, _ = inflate(B, np.ascontiguousarray(pts[::-1]), ns, 0)
    assert n_new == len(full)
    gs.assert_same_state(gs.state(A), gs.state(B), "cap 0")
    # getCloud with cap below the total
    cloud = A.getCloud()
    total = C.c_uint64(0)
    part = np.full((len(cloud), 3), -77.0)
    cap = len(cloud) // 2
    A._check(lib.mplx_grid_get_cloud(A.h, part.ctypes.data, cap, C.byref(total)))
    assert total.value == len(cloud) > 10 and np.array_equal(part[:cap], cloud[:cap]) and np.all(part[cap:] == -77.0)
    # n == 0: nothing happens; n_ns == 0: the map is marked, nothing inflates, new_obs is empty
    before = gs.state(A)
    n_new, _ = inflate(A, np.zeros((0, 3)), ns, 4)
    assert n_new == 0
    A._check(lib.mplx_grid_add_cloud(A.h, 0, None))
    gs.assert_same_state(before, gs.state(A), "n == 0")
    for g in (A, O):
        g.clear()
    n_new, _ = inflate(A, pts, np.zeros((0, 3), dtype=np.int32), 4)
    assert n_new == 0 and len(O.add_cloud(pts, np.zeros((0, 3), dtype=np.int32))) == 0
    s = gs.state(A)
    gs.assert_same_state(gs.state(O), s, "n_ns == 0")
    assert s[1].any() and not s[2].any()
    # ... and the scratch is intact afterwards
    assert np.array_equal(A.addCloud(pts, ns), O.add_cloud(pts, ns))
    gs.assert_same_state(gs.state(O), gs.state(A), "after n_ns == 0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINGLE_POINT_SCENES)
def test_device_grid_on_one_point_clouds(name):
    """addCloud(pts) and addCloud(pts, ns) with n == 1"""
    run_single_points(name, parties())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NONFINITE_SCENES)
def test_device_skips_non_finite_points(name):
    """The device's f64 -> i32 convert gives 0 for NaN where x86 gives INT_MIN: without the explicit range test in
    grid_cell_of a NaN coordinate lands in cell 0 of its axis, and an all-NaN point occupies cell (0, 0, 0)."""
    run_nonfinite(name, parties())


# ---------------------------------------------------------------------------------------------------------------- the C++ shim
DRIVER_SCENES = {"neg_unaligned": ((3, 2, 1), (2, 1, 1)), "flat": ((3, 2, 0), (2, 1, 0))}  # allocate: cells added, cells the origin moves down


def driver_inputs(name):
    sc = SCENES[name]
    rng = np.random.default_rng(31)
    r = gs.f32(sc["res"])
    add, down = DRIVER_SCENES[name]
    flat = sc["size"][2] == 0.0
    size2 = tuple(0.0 if (flat and i == 2) else (sc["cells"][i] + add[i] + 0.5) * r for i in range(3))
    ori2 = tuple(sc["origin"][i] - down[i] * r for i in range(3))
    pts1 = gs.make_points(rng, sc["origin"], sc["cells"], sc["res"], 150)
    pts2 = gs.make_points(rng, sc["origin"], sc["cells"], sc["res"], 100)
    return sc, size2, ori2, pts1, pts2


def driver_args(tmp_path, name):
    sc, size2, ori2, pts1, pts2 = driver_inputs(name)
    path = str(tmp_path / (name + "_cloud.bin"))
    np.concatenate([pts1, pts2]).tofile(path)
    return [repr(float(v)) for v in sc["origin"] + sc["size"] + (gs.f32(sc["res"]),) + size2 + ori2] + [path, str(len(pts1)), str(len(pts2))]


@pytest.fixture(scope="module")
def grid_driver(tmp_path_factory):
    from tests import test_cpp_shim
    return test_cpp_shim.build_driver(tmp_path_factory.mktemp("voxel_grid_driver"), "voxel_grid_driver")


def test_voxel_grid_driver_compiles_links_and_fails_loudly_without_gpu(grid_driver, tmp_path):
    from mpl_ros_amd import _capi
    h = C.c_void_p()
    if _capi.load().mplx_ctx_create(0, C.byref(h)) == _capi.OK:  # (the library's own view of "is there a GPU")
        _capi.load().mplx_ctx_destroy(h)
        pytest.skip("GPU present")
    out = subprocess.run([grid_driver] + driver_args(tmp_path, "flat"), capture_output=True, text=True)
    assert out.returncode == 3 and "no HIP device" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DRIVER_SCENES))
def test_shim_voxel_grid_matches_oracle(grid_driver, tmp_path, name):
    """tests/cpp/voxel_grid_driver.cpp: one fixed sequence through the C++ VoxelGrid of include/mpl_shim, step by step"""
    sc, size2, ori2, pts1, pts2 = driver_inputs(name)
    out = subprocess.run([grid_driver] + driver_args(tmp_path, name), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.strip().splitlines()]
    ring = [(x, y, z) for x in (-3, 0, 3) for y in (-3, 0, 3) for z in (-3, 0, 3) if (x, y, z) != (0, 0, 0)]
    assert ring == gs.NS_RING3
    O = orc.Grid(sc["origin"], sc["size"], sc["res"])

    def fill_clear():
        O.fill(2, 1); O.fill(0, 0, 0); O.fill(-1, 0); O.fill(1, 1, 400); O.clear(3, 2)

    steps = [("constructor", lambda: None), ("addCloud", lambda: O.add_cloud(pts1)), ("addCloud_ns", lambda: O.add_cloud(pts2, gs.NS_18)),
             ("decay", O.decay), ("fill_clear", fill_clear), ("addCloud_ns_again", lambda: O.add_cloud(pts2, gs.NS_18)),
             ("allocate", lambda: O.allocate(size2, ori2)), ("allocate_same", lambda: O.allocate(size2, ori2)),
             ("addCloud_ring", lambda: O.add_cloud(pts1, gs.NS_RING3)), ("clear", O.clear)]
    assert [l["step"] for l in lines] == [s for s, _ in steps]
    flags = {"allocate": 1, "allocate_same": 0}
    seen_obs = 0
    for l, (step, run) in zip(lines, steps):
        r = run()
        dim, ori, res = O.info()
        for key, inflated in (("map", False), ("inflated", True)):
            m = l[key]
            assert tuple(m["dim"]) == dim and tuple(m["origin"]) == ori and np.float32(m["res"]) == np.float32(res), (step, key)
            assert np.array_equal(np.frombuffer(bytes.fromhex(m["data"]), dtype=np.int8), O.get_map(inflated)), (step, key)
        cloud = np.array(l["cloud"], dtype=np.float64).reshape(-1, 3)
        want = O.get_cloud()
        assert cloud.shape == want.shape and np.array_equal(cloud.view(np.uint64), want.view(np.uint64)), step
        if isinstance(r, np.ndarray):
            assert np.array_equal(np.array(l["new_obs"], dtype=np.int32).reshape(-1, 3), r), step
            seen_obs += len(r)
        else:
            assert l["new_obs"] == []
        if step in flags:
            assert l["flag"] == flags[step] and bool(r) == bool(flags[step])
    assert seen_obs > 100
