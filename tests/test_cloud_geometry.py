"""The point-cloud planner off the origin, in all four control kinds, at the edges of its index and of its sampling.

Every other test of this planner keeps its cloud in the positive octant within some 31 m of the origin and runs ACC or JRK states.
Here the clouds are cloud_scenes.SCENES: boxes with all-negative, mixed-sign and far-away origins (1e3, -1e4, 1e5 m: a float32 ulp
is 6e-5, 1e-3 and 8e-3 m there, so the radius filter's float arithmetic decides primitives), radii that are exact in float32 and radii
that round, points on the faces of the index's cells and on the rim of the strict radius filter, index tables of 1 to 4096 buckets,
points that are not finite, and the sampling edges of one expansion; VEL, ACC, JRK and SNP states.  The device is compared bit for
bit (cloud_compare._compare_succ / _compare_plan) with the checker in brute mode, which has no index that could be wrong in the same
way.  The regimes a test is meant to reach are asserted from the checker alone, so inputs that drift out of a regime fail.

CPU part: the table covers what it is meant to cover, grid and brute mode of the checker agree, every regime holds.
GPU part: get_succ over the table, re-indexing on one handle, plans per control kind, search outcomes, slot reuse in a batch."""
import ctypes as C
import math

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd.ellipsoid import control_lattice, state13
from oracle import orc
from tests import cloud_checker as K
from tests import cloud_scenes as S
from tests.cloud_compare import _compare_plan, _compare_succ

CN = {orc.VEL: "VEL", orc.ACC: "ACC", orc.JRK: "JRK", orc.SNP: "SNP"}
L = S.LAUNCH
SWEEP = ("neg_r05", "mixed_r0625", "far1e3_r03", "farm1e4_r005", "far1e5_r2", "eq_origin", "eq_1e3", "eq_m1e4", "eq_1e5", "cell_faces",
         "knife_edge", "door_1e3")
INDEX = tuple(f"index_{n}" for n in S.INDEX_SIZES) + ("index_copies", "nonfinite")
SAMPLING = ("nu_1", "nu_256", "ceil_edge", "long_261", "pairs_256_257", "mid_box")
FAR_EQ = ("eq_1e3", "eq_m1e4", "eq_1e5")
DOOR = "door_1e3"


def cases(names):
    return [pytest.param(n, c, id=f"{n}-{CN[c]}") for n in names for c in S.SCENES[n]["controls"]]


# ---------------------------------------------------------------------------------------------------------------- the checker's side
_ref = {}


def reference(name, control):
    """(checker in brute mode, its get_succ records per state) of a scene: computed once, shared, never modified"""
    if (name, control) not in _ref:
        pts, states = S.build(name, control)
        ck = S.checker(S.SCENES[name], control, pts)
        _ref[(name, control)] = (ck, [ck.get_succ(s) for s in states])
    return _ref[(name, control)]


def valid_of(recs):
    return np.array([[ok for ok, *_ in rs] for rs in recs], dtype=bool)


def same_records(a, b):
    return all(x[0] == y[0] and np.array_equal(x[1], y[1]) and x[2] == y[2] and x[3] == y[3] for ra, rb in zip(a, b) for x, y in zip(ra, rb))


class Cloud64(K.Cloud):
    """the cloud with the radius filter in float64 on the double coordinates: E2 without its float32 arithmetic"""

    def blocked_at(self, d, acc):
        v0, v1, v2 = self.pd[:, 0] - d[0], self.pd[:, 1] - d[1], self.pd[:, 2] - d[2]
        cand = np.flatnonzero((v0 * v0 + v1 * v1) + v2 * v2 < self.r * self.r)
        if len(cand) == 0:
            return False
        Cm, _ = K.ellipsoid_C(self.axe, acc)
        return bool(np.any(K.inside(K.inverse3(Cm), d, self.pd[cand])))


def filter_flips(name, control=orc.ACC):
    """primitives whose validity differs between the float32 radius filter and a float64 one"""
    sc = S.SCENES[name]
    pts, states = S.build(name, control)
    ck64 = S.checker(sc, control, pts, cloud=Cloud64(pts, sc["r"], sc["ori"], sc["dim"], brute=True))
    v32 = valid_of(reference(name, control)[1])
    return int((v32 != valid_of([ck64.get_succ(s) for s in states])).sum())


def stage(ck, s13, i):
    """how far primitive (s13, U[i]) gets in get_succ, from the checker's pieces: (tn != curr, validate_primitive, the three box
    samples of E1, n of E6)"""
    lib = orc.lib()
    pr = S.primitive(ck, s13, i)
    tn = orc.Waypoint()
    lib.orc_primitive_evaluate(C.byref(pr), ck.dt, C.byref(tn))
    tn.control = ck.control
    moves = K.key_of(tn) != K.key_of(K.state_wp(s13, ck.control))
    validated = bool(lib.orc_validate_primitive(C.byref(pr), ck.v_max, ck.a_max, ck.j_max))
    box = [K.in_bbox(ck.cloud.planes, list(S.sample(pr, k * (ck.dt / 2))[0])) for k in range(3)]
    return moves, validated, box, S.n_of(pr, ck.dt, ck.cloud.r)


def pair_total(ck, s13):
    """(primitive, ellipsoid) pairs of one expansion: n + 1 of every primitive that reaches the point test"""
    tot = 0
    for i in range(len(ck.U)):
        moves, validated, box, n = stage(ck, s13, i)
        if moves and validated and all(box):
            tot += n + 1
    return tot


def resting_inside(r, centre, pts):
    """E3 at a sample with zero acceleration"""
    Cm, _ = K.ellipsoid_C((r, r, K.H_AXE), (0.0, 0.0, 0.0))
    return K.inside(K.inverse3(Cm), list(centre), np.asarray(pts, dtype=np.float64).reshape(-1, 3))


def e2_candidate(r, centre, p):
    """E2: float32 centre, point, differences, squares and sums against float32(r_f r_f)"""
    rf = np.float32(r)
    c, q = np.asarray(centre, dtype=np.float64).astype(np.float32), np.asarray(p, dtype=np.float64).astype(np.float32)
    dx, dy, dz = q[0] - c[0], q[1] - c[1], q[2] - c[2]
    return bool((dx * dx + dy * dy) + dz * dz < np.float32(float(rf) * float(rf)))


# ---- the regimes, one function each: asserted in the CPU part, and again by the GPU test that relies on them
def regime_knife_edge():
    """states 0..3: the point is inside the ellipsoid at c = p + (0.5, 0.5, 0) of input (2, 2, 0) and not a candidate of the radius
    filter, farther than r from every other tested centre, and the primitive is free; states 4..7 (one ulp inward): a candidate, blocked"""
    sc = S.SCENES["knife_edge"]
    ck, recs = reference("knife_edge", orc.VEL)
    pts, states = S.build("knife_edge", orc.VEL)
    i = [tuple(u) for u in ck.U.tolist()].index((2.0, 2.0, 0.0))
    for k, s13 in enumerate(states):
        (d0, _, _), (c, _, _) = S.ellipsoids(ck, s13, i)
        assert np.array_equal(c, s13[0:3] + np.array([0.5, 0.5, 0.0])) and np.all(c * 64 == np.round(c * 64))
        assert resting_inside(sc["r"], c, pts[k])[0]
        assert e2_candidate(sc["r"], c, pts[k]) == (k >= 4)
        for j in range(len(ck.U)):
            for d, _, _ in S.ellipsoids(ck, s13, j):
                assert np.array_equal(d, c) or np.linalg.norm(pts[k] - d) > sc["r"] + 0.1
        for k2 in range(len(pts)):
            assert k2 == k or np.linalg.norm(pts[k2] - s13[0:3]) > 2.5
        assert recs[k][i][0] == (k < 4)
    offs = {tuple(np.round(pts[k] - states[k, 0:3] - np.array([0.5, 0.5, 0.0]), 9)) for k in range(4)}
    assert offs == {(0.625, 0.0, 0.0), (0.375, 0.5, 0.0)}
    assert {tuple(np.sign(states[k, 0:2])) for k in range(4)} == {(1, 1), (-1, -1), (1, -1), (-1, 1)}


def regime_cell_faces():
    """every point is within 1 float32 ulp of a cell corner k L; over the corners each axis has a point in cell k and one in cell k - 1, at
    k > 0, k < 0 and k = 0; every state's t = 0 centre is in a cell next to (or equal to) the point's on each axis, all 27 relative
    positions of point cell and centre cell occur, and the point decides at least one primitive of every state"""
    sc = S.SCENES["cell_faces"]
    ck, recs = reference("cell_faces", orc.ACC)
    pts, states = S.build("cell_faces", orc.ACC)
    rf = float(np.float32(sc["r"]))
    sides, rel = set(), set()
    for c, corner in enumerate(S.FACE_CORNERS):
        for ax in range(3):
            x = np.float32(pts[c, ax])
            assert abs(float(x) - corner[ax] * rf * S.CELL_MARGIN) <= float(np.spacing(np.float32(abs(corner[ax]) * rf * S.CELL_MARGIN)))
            u = S.cell_of(x, sc["r"])
            assert u in (corner[ax], corner[ax] - 1)
            sides.add((int(np.sign(corner[ax])), u - corner[ax]))
        for s13 in states[8 * c:8 * c + 8]:
            d = tuple(S.cell_of(s13[ax], sc["r"]) - S.cell_of(pts[c, ax], sc["r"]) for ax in range(3))
            assert max(abs(x) for x in d) <= 1
            rel.add(d)
    assert sides == {(s, side) for s in (-1, 0, 1) for side in (-1, 0)}
    assert len(rel) >= 20 and {d for d in rel if 0 not in d} == {(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)}
    empty = S.checker(sc, orc.ACC, [])
    for k, s13 in enumerate(states):
        v = valid_of([recs[k]])[0]
        assert 0 < v.sum() < valid_of([empty.get_succ(s13)])[0].sum()


def regime_small_index(name):
    """n <= 8: every point of the cloud, alone, blocks a primitive that is free in the empty box"""
    sc = S.SCENES[name]
    control = sc["controls"][0]
    pts, states = S.build(name, control)
    assert len(pts) == sc["n_pts"] <= 8
    free = valid_of([S.checker(sc, control, []).get_succ(s) for s in states])
    for p in pts:
        one = S.checker(sc, control, p[None, :])
        assert (valid_of([one.get_succ(s) for s in states]) != free).any()


def regime_sampling(name):
    sc = S.SCENES[name]
    control = sc["controls"][0]
    ck, recs = reference(name, control)
    pts, states = S.build(name, control)
    v = valid_of(recs)
    if name == "nu_1":
        assert len(ck.U) == 1
    elif name == "nu_256":
        assert len(ck.U) == 256 and len({tuple(u) for u in ck.U.tolist()}) == 256
    elif name == "ceil_edge":  # max_v dt / r is the integer 2; the middle ellipsoid alone decides input 0
        pr = S.primitive(ck, states[0], 0)
        q = S.max_vel(pr) * ck.dt / sc["r"]
        assert q == 2.0 and S.n_of(pr, ck.dt, sc["r"]) == 2
        for k, s13 in enumerate(states):
            el = S.ellipsoids(ck, s13, 0)
            assert len(el) == 3 and [resting_inside(sc["r"], d, pts[k])[0] for d, _, _ in el] == [False, k % 2 == 0, False]
            for t in (ck.dt / 3, 2 * ck.dt / 3):  # (the centres a sampling with n = 3 would add)
                assert np.linalg.norm(S.sample(pr, t)[0] - states[0, 0:3] - (pts[0] - states[0, 0:3])) > sc["r"]
            assert v[k, 0] == (k % 2 == 1)
    elif name == "long_261":  # n = 260: ellipsoids 256..260 are staged in a second chunk
        assert stage(ck, states[0], 0)[3] == 260
        assert [bool(x) for x in v[:, 0]] == [False, True, False, True, False, True]
        assert sum(S.n_of(S.primitive(ck, states[0], i), ck.dt, sc["r"]) + 1 for i in range(2)) > 256
    elif name == "pairs_256_257":
        tot = [pair_total(ck, s13) for s13 in states]
        assert tot == [256, 256, 257, 257, 256, 256, 257, 257]
        last = [1 if k % 4 < 2 else 2 for k in range(len(states))]  # (the primitive whose last ellipsoid is pair 255 / 256)
        assert [bool(v[k, last[k]]) for k in range(len(states))] == [k % 2 == 0 for k in range(len(states))]
        for k, s13 in enumerate(states):
            hold = [bool(resting_inside(sc["r"], d, pts[k])[0]) for d, _, _ in S.ellipsoids(ck, s13, last[k])]
            assert hold == [False] * (len(hold) - 1) + [k % 2 == 1]
    elif name == "mid_box":  # states 0..3: input k starts and ends inside the box and leaves it at t = dt / 2 only
        for k in range(4):
            moves, validated, box, n = stage(ck, states[k], k)
            assert moves and validated and box == [True, False, True] and not v[k, k]
        assert stage(ck, states[4], 0)[2] == [True, True, True] and v[4, 0] and v[5].sum() >= 3
    return v


def regime_every_n(ck, states):
    """the n of E6 over the primitives of `states` that move"""
    return [stage(ck, s, i)[3] for s in states for i in range(len(ck.U)) if stage(ck, s, i)[0]]


# ---------------------------------------------------------------------------------------------------------------- CPU: the table
def test_scene_table_covers_what_the_sweep_is_for():
    G = S.SCENES
    assert set(SWEEP + INDEX + SAMPLING) == set(G)
    # box origins: all negative, mixed sign, about 1e3, -1e4 and 1e5 m away; none on the index's cell lattice
    assert any(all(o < 0 for o in g["ori"]) for g in G.values())
    assert any(min(g["ori"]) < 0 < max(g["ori"]) for g in G.values())
    assert any(900 <= max(g["ori"]) <= 1100 for g in G.values())
    assert any(-11000 <= min(g["ori"]) <= -9000 for g in G.values())
    assert any(9e4 <= max(g["ori"]) <= 1.1e5 for g in G.values())
    for g in G.values():
        cell = float(np.float32(g["r"])) * S.CELL_MARGIN
        assert all(abs(o / cell - round(o / cell)) > 1e-3 for o in g["ori"])
    # radii: 0.5 and 0.625 are float32 values, 0.3 and 0.05 round, 2.0 makes n = 1 the rule
    assert {0.5, 0.625, 0.3, 0.05, 2.0} <= {g["r"] for g in G.values()}
    assert float(np.float32(0.625)) == 0.625 and float(np.float32(0.3)) != 0.3 and float(np.float32(0.05)) != 0.05
    for r in (0.5, 0.625, 0.3, 0.05, 2.0):
        assert any(g["r"] == r and set(g["controls"]) == set(S.ALL_KINDS) for g in G.values())  # ... each in all four control kinds
    big = S.SCENES["far1e5_r2"]
    ns = regime_every_n(S.checker(big, orc.ACC, []), S.build("far1e5_r2", orc.ACC)[1])
    assert sum(n == 1 for n in ns) > len(ns) / 2
    # the far scenes of the float-filter regime and their control at the origin
    assert all(max(abs(o) for o in G[n]["ori"]) >= 900 for n in FAR_EQ) and max(abs(o) for o in G["eq_origin"]["ori"]) < 10
    # index sizes: n = 1, 2, 3, 5, 8, both sides of the scan's slice change (1024 -> 2048 buckets), about 3000, and one crowded bucket
    sizes = {len(S.build(n, G[n]["controls"][0])[0]) for n in INDEX if n.startswith("index_") and n != "index_copies"}
    assert sizes == set(S.INDEX_SIZES) and {1, 2, 3, 5, 8, 1023, 1024, 1025} <= sizes and any(2500 <= n <= 3500 for n in sizes)
    pts = S.build("index_copies", orc.ACC)[0]
    uniq, count = np.unique(pts, axis=0, return_counts=True)
    assert count.max() == 4097 and len(uniq) > 40  # (the copied point and its original)
    # every cloud a brute-mode checker is built on stays under 5 000 points, every case under 150 states
    for name, g in G.items():
        for c in g["controls"]:
            pts, states = S.build(name, c)
            assert len(pts) < 5000 and len(states) <= 150
            assert 40 <= len(states) or name in ("knife_edge", "ceil_edge", "long_261", "pairs_256_257", "mid_box", "nu_256") or len(pts) <= 8
    # not finite: NaN, +-inf, 1e300 (float32 inf) and 1e30 among finite points
    bad = S.build("nonfinite", orc.ACC)[0]
    bad = bad[~(np.abs(bad) < 1e30).all(axis=1)]
    assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any() and (bad == 1e300).any() and (bad == 1e30).any()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e300)) and np.isfinite(np.float32(1e30)) and len(bad) == 42
    # the four control kinds all run somewhere in every family
    for fam in (SWEEP, INDEX):
        assert {c for n in fam for c in G[n]["controls"]} == set(S.ALL_KINDS) or fam is INDEX
    assert {orc.ACC, orc.JRK, orc.SNP} <= {c for n in INDEX for c in G[n]["controls"]}


@pytest.mark.parametrize("name,control", cases([n for n in SWEEP + INDEX + SAMPLING if n != "nonfinite"]))
def test_grid_and_brute_mode_of_the_checker_agree(name, control):
    pts, states = S.build(name, control)
    grid = S.checker(S.SCENES[name], control, pts, brute=False)
    assert grid.cloud.grid and not reference(name, control)[0].cloud.grid
    assert same_records([grid.get_succ(s) for s in states], reference(name, control)[1])


def test_grid_and_brute_mode_agree_on_the_office():
    rng = np.random.default_rng(5)
    pts = S.office()
    U = control_lattice(L["u_max"], 1, True, 20.0)
    st = np.zeros((300, 13))
    st[:, 0:3] = rng.uniform((6.5, 12.5, 0.2), (30.5, 16.5, 1.4), size=(300, 3))
    st[:, 3:6] = rng.uniform(-6, 6, size=(300, 3))
    cks = [K.Checker(K.Cloud(pts, L["r"], S.ORI, S.DIM, brute=b), orc.ACC, U, L["dt"], v_max=L["v_max"], a_max=L["a_max"]) for b in (False, True)]
    a, b = [[ck.get_succ(s) for s in st] for ck in cks]
    assert same_records(a, b) and 0 < valid_of(a).sum() < valid_of(a).size
    assert cks[1].cloud.tests > 20 * cks[0].cloud.tests  # (brute mode really looked at every point)


def test_brute_mode_accepts_points_that_are_not_finite_and_they_change_no_decision():
    for control in S.SCENES["nonfinite"]["controls"]:
        sc = S.SCENES["nonfinite"]
        pts, states = S.build("nonfinite", control)
        fin, _ = S.build_nonfinite(sc, control, finite_only=True)
        assert len(pts) == len(fin) + 42
        ck = S.checker(sc, control, fin)
        assert same_records([ck.get_succ(s) for s in states], reference("nonfinite", control)[1])
        # a finite point at the place of each of them would have blocked: the other coordinates are a state's own position
        k = int(np.flatnonzero(np.isnan(pts).any(axis=1))[0])
        at = [s for s in states if np.sum(pts[k] == s[0:3]) >= 1]
        one = S.checker(sc, control, np.array([at[0][0:3]]))
        assert not valid_of([one.get_succ(at[0])]).any()


# ---------------------------------------------------------------------------------------------------------------- CPU: the regimes
def test_far_equator_scenes_are_where_the_float32_filter_decides():
    flips = {n: filter_flips(n) for n in FAR_EQ + ("eq_origin",)}
    print(flips)
    assert all(flips[n] >= 8 for n in FAR_EQ) and flips["eq_origin"] == 0
    for n in FAR_EQ + ("eq_origin",):  # resting states, n = 1
        ck, recs = reference(n, orc.ACC)
        states = S.build(n, orc.ACC)[1]
        assert not states[:, 3:12].any() and set(regime_every_n(ck, states[:5])) == {1}


def test_knife_edge_points_are_inside_the_ellipsoid_and_outside_the_strict_filter():
    regime_knife_edge()


def test_cell_face_points_fall_on_both_sides_of_a_face():
    regime_cell_faces()


@pytest.mark.parametrize("name", [f"index_{n}" for n in (1, 2, 3, 5, 8)])
def test_small_index_points_are_within_reach_of_tested_ellipsoids(name):
    regime_small_index(name)


@pytest.mark.parametrize("name", SAMPLING)
def test_sampling_edges_are_reached(name):
    regime_sampling(name)


def test_sample_counts_reach_their_edges():
    ns = []
    for name, control in (("neg_r05", orc.ACC), ("farm1e4_r005", orc.JRK), ("far1e5_r2", orc.VEL), ("long_261", orc.VEL)):
        ns += regime_every_n(reference(name, control)[0], S.build(name, control)[1][:10])
    assert min(ns) == 1 and max(ns) >= 257 and any(10 <= n <= 60 for n in ns)  # (n = 0 cannot pass tn != curr: E6)


@pytest.mark.parametrize("name,control", cases(SWEEP + INDEX + SAMPLING))
def test_every_get_succ_case_has_valid_and_blocked_successors(name, control):
    v = valid_of(reference(name, control)[1])
    assert 0 < v.sum() < v.size
    free = S.checker(S.SCENES[name], control, [])
    if name != "mid_box":  # (its rejections are the box's): the cloud itself blocks primitives that the empty box lets pass
        assert v.sum() < valid_of([free.get_succ(s) for s in S.build(name, control)[1]]).sum()


# ---- plans
class PlanChecker(K.Checker):
    """the checker with the plan() keywords that the shared comparison does not pass"""
    extra = {}

    def plan(self, start, goal, **kw):
        return super().plan(start, goal, **dict(kw, **self.extra))


def door_checker(control, hid=False, pts=None):
    sc = S.SCENES[DOOR]
    ck = S.checker(sc, control, S.build(DOOR, control)[0] if pts is None else pts, cls=PlanChecker)
    ck.extra = dict(heur_ignore_dynamics=hid)
    return ck


def door_query(pair):
    sc = S.SCENES[DOOR]
    return state13(S.at(sc, pair[0])), state13(S.at(sc, pair[1]))


def checker_plan(ck, start, goal, max_num):
    return ck.plan(start, goal, eps=L["eps"], tol_pos=L["tol"][0], tol_vel=L["tol"][1], tol_acc=L["tol"][2], max_num=max_num)


PLAN_CASES = [(c, p, h) for c in S.ALL_KINDS for p, hs in (("hard", (False, True)), ("easy", (False, True)), ("diag", (True,))) for h in hs]
PLANS = [pytest.param(c, p, h, id=f"{CN[c]}-{p}-{'nodyn' if h else 'dyn'}") for c, p, h in PLAN_CASES]
E8_POINT = (-0.45, 0.0, 0.04)  # from the start: inside its resting ellipsoid (r = 0.5, h = 0.1)


def e8_cloud():
    sc = S.SCENES[DOOR]
    start = np.array(S.at(sc, sc["pairs"]["easy"][0]))
    return np.concatenate([S.build(DOOR, orc.ACC)[0], [start + np.array(E8_POINT)]])


def test_door_plans_on_the_checker_cover_the_outcomes():
    sc = S.SCENES[DOOR]
    assert max(abs(o) for o in sc["ori"]) >= 900
    got = {}
    for c, p, h in PLAN_CASES:
        r = checker_plan(door_checker(c, h), *door_query(sc["pairs"][p]), 400)
        assert r["status"] in (0, 3) and 3 <= len(r["expanded"]) <= 400
        got[(c, p, h)] = (r["status"], len(r["expanded"]))
    for c in S.ALL_KINDS:  # every kind reaches a goal, and the heuristic's mode changes the search
        assert any(s == 0 for (c2, _, _), (s, _) in got.items() if c2 == c)
        assert any(got[(c, p, False)] != got[(c, p, True)] for p in ("hard", "easy"))
    assert any(s == 3 for s, _ in got.values())
    # the hard pair cannot go straight: the segment from start to goal meets the wall (x = 6, outside 2 < y < 4)
    a, b = sc["pairs"]["hard"]
    assert a[0] < 6.0 < b[0] and a[1] == b[1] and not 2.0 < a[1] < 4.0
    # the sealed closet: OPEN runs empty after a few dozen expansions
    ck = door_checker(orc.VEL)
    r = checker_plan(ck, state13(S.at(sc, sc["closet"])), state13(S.at(sc, sc["pairs"]["hard"][0])), 400)
    assert r["status"] == 1 and 20 <= len(r["expanded"]) <= 300
    # a start inside the goal tolerance
    r = checker_plan(ck, *door_query(S.REUSE_QUERIES[3]), 400)
    assert r["status"] == 0 and r["cost"] == 0.0 and r["expanded"] == []
    # E8: a point inside the start's own ellipsoid; the search still leaves the start
    start, goal = door_query(sc["pairs"]["easy"])
    assert resting_inside(sc["r"], start[0:3], start[0:3] + np.array(E8_POINT))[0]
    ck = door_checker(orc.ACC, pts=e8_cloud())
    first = valid_of([ck.get_succ(start)])[0]
    assert 0 < first.sum() < valid_of([door_checker(orc.ACC).get_succ(start)])[0].sum()
    r = checker_plan(ck, start, goal, 400)
    assert r["status"] == 0 and len(r["expanded"]) > 3


def reuse_reference():
    """the 16 queries of the slot-reuse batch on the checker: [(status, expansions)]"""
    if "reuse" not in _ref:
        ck = door_checker(orc.VEL, True)
        _ref["reuse"] = [checker_plan(ck, *door_query(q), S.REUSE_MAX_NUM) for q in S.REUSE_QUERIES]
    return _ref["reuse"]


def test_slot_reuse_queries_mix_the_four_outcomes():
    res = reuse_reference()
    kinds = ["goal" if r["status"] == 0 and not r["expanded"] else {0: "reached", 1: "no path", 3: "capped"}[r["status"]] for r in res]
    print(kinds)
    assert len(res) == 16 and all(kinds.count(k) >= 2 for k in ("reached", "capped", "no path", "goal"))
    assert all(kinds[i] != kinds[i + 1] for i in range(0, 4))  # (mixed: a slot's next query is of another kind)
    assert len({kinds[q] for q in range(0, 16, 4)}) >= 2


# ---------------------------------------------------------------------------------------------------------------- GPU
def configure(pl, sc, control):
    pl.set_control(control)
    pl.set_u(S.lattice(sc, control))
    pl.set_dt(sc["dt"]); pl.set_vmax(sc["v_max"]); pl.set_amax(sc["a_max"]); pl.set_jmax(sc["j_max"]); pl.set_w(10.0)
    return pl


def device(sc, control, pts):
    from mpl_ros_amd.ellipsoid import EllipsoidPlanner
    pl = EllipsoidPlanner(False)
    pl.set_map(pts, sc["r"], sc["ori"], sc["dim"])
    return configure(pl, sc, control)


def compare_scene(name, control):
    """get_succ_batch of the scene's states on the device against brute mode, bit for bit; both outcomes occur"""
    pts, states = S.build(name, control)
    ck = reference(name, control)[0]
    n_valid = _compare_succ(device(S.SCENES[name], control, pts), ck, states)
    assert 0 < n_valid < states.shape[0] * len(ck.U)


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", cases(SWEEP))
def test_get_succ_over_the_scene_table(name, control):
    if name in FAR_EQ:
        assert filter_flips(name, control) >= 8
    if name == "knife_edge":
        regime_knife_edge()
    if name == "cell_faces":
        regime_cell_faces()
    compare_scene(name, control)


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", cases(INDEX))
def test_get_succ_index_sizes_and_points_that_are_not_finite(name, control):
    sc = S.SCENES[name]
    if sc.get("n_pts", 9) <= 8:
        regime_small_index(name)
    if name == "nonfinite":
        pts = S.build(name, control)[0]
        assert np.isnan(pts).any() and np.isinf(pts).any() and (np.abs(pts) == 1e300).any()
    compare_scene(name, control)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SAMPLING)
def test_get_succ_sampling_edges(name):
    regime_sampling(name)
    compare_scene(name, S.SCENES[name]["controls"][0])


@pytest.mark.gpu
def test_set_map_again_on_one_handle_large_small_empty_large():
    """re-indexing: 3001 points (4096 buckets), 12 of them (16 buckets), none, 3001 again, on one handle; after each set_map the
    successors equal a fresh handle's and the checker's"""
    name, control = "index_3001", orc.JRK
    sc = S.SCENES[name]
    large, states = S.build(name, control)
    small = S.build_surface(sc, control)[0][:12]  # (the points on the ellipsoids of the first three states)
    free = valid_of([S.checker(sc, control, []).get_succ(s) for s in states])
    v_small = valid_of([S.checker(sc, control, small).get_succ(s) for s in states])
    assert valid_of(reference(name, control)[1]).sum() < v_small.sum() < free.sum()
    pl = device(sc, control, large)
    for pts in (large, small, np.zeros((0, 3)), large):
        pl.set_map(pts, sc["r"], sc["ori"], sc["dim"])
        ck = S.checker(sc, control, pts)
        got = pl.get_succ_batch(states)
        fresh = device(sc, control, pts).get_succ_batch(states)
        assert all(np.array_equal(a, b) for a, b in zip(got, fresh))
        n_valid = _compare_succ(pl, ck, states)
        assert n_valid == (free.sum() if len(pts) == 0 else v_small.sum() if len(pts) == 12 else valid_of(reference(name, control)[1]).sum())


def door_device(control, hid, pts=None, slots=1):
    pl = device(S.SCENES[DOOR], control, S.build(DOOR, control)[0] if pts is None else pts)
    pl.set_capacity(slots, slots << 18, slots << 20, slots << 18)
    pl.set_epsilon(L["eps"])
    pl.set_tol(*L["tol"])
    pl.set_heur_ignore_dynamics(hid)
    return pl


@pytest.mark.gpu
@pytest.mark.parametrize("control,pair,hid", PLANS)
def test_door_plan_per_control_kind(control, pair, hid):
    """a far-away room with a wall and a doorway, VEL / ACC / JRK / SNP, heur_ignore_dynamics off and on: the plan reaches the goal or
    stops at 400 expansions, and equals the checker's in every field"""
    start, goal = door_query(S.SCENES[DOOR]["pairs"][pair])
    r, c = _compare_plan(door_device(control, hid), door_checker(control, hid), start, goal, max_num=400)
    assert r["status"] in (_capi.PLAN_OK, _capi.PLAN_MAX_EXPAND) and 3 <= r["n_expanded"] <= 400
    assert (r["status"] == _capi.PLAN_MAX_EXPAND) == (r["n_expanded"] == 400 and c["status"] == 3)


@pytest.mark.gpu
def test_sealed_closet_has_no_path():
    sc = S.SCENES[DOOR]
    r, c = _compare_plan(door_device(orc.VEL, False), door_checker(orc.VEL), state13(S.at(sc, sc["closet"])), state13(S.at(sc, sc["pairs"]["hard"][0])),
                         max_num=400)
    assert r["status"] == _capi.PLAN_NO_PATH and 20 <= r["n_expanded"] <= 300 and math.isinf(r["cost"])


@pytest.mark.gpu
@pytest.mark.parametrize("control", S.ALL_KINDS)
def test_start_inside_the_goal_tolerance(control):
    start, goal = door_query(S.REUSE_QUERIES[3])
    c = checker_plan(door_checker(control), start, goal, 400)
    assert c["status"] == 0 and c["cost"] == 0.0 and c["expanded"] == []
    pl = door_device(control, False)
    pl.set_max_num(400)
    assert pl.plan(start, goal)
    r = pl.result()
    assert r["status"] == _capi.PLAN_OK and r["cost"] == 0.0 and r["n_expanded"] == 0 and r["traj_len"] == 0
    assert pl.get_traj() is None


@pytest.mark.gpu
def test_start_whose_own_ellipsoid_holds_a_point_still_plans():
    """E8: the start is always free.  The point is inside the start's resting ellipsoid; the primitives whose first ellipsoid tilts away
    from it pass, and the plan reaches the goal"""
    sc = S.SCENES[DOOR]
    start, goal = door_query(sc["pairs"]["easy"])
    assert resting_inside(sc["r"], start[0:3], start[0:3] + np.array(E8_POINT))[0]
    pts = e8_cloud()
    r, c = _compare_plan(door_device(orc.ACC, False, pts=pts), door_checker(orc.ACC, pts=pts), start, goal, max_num=400)
    assert r["status"] == _capi.PLAN_OK and r["n_expanded"] > 3


@pytest.mark.gpu
def test_sixteen_queries_on_three_slots_equal_single_queries_and_the_checker():
    """n > n_slots: a workgroup takes its next query through the batch counter and reuses its pools, its OPEN buckets and its
    expansion state.  Reached, capped, no-path and start-is-goal queries in mixed order"""
    ref = reuse_reference()
    starts, goals = [np.array(x) for x in zip(*[door_query(q) for q in S.REUSE_QUERIES])]
    pl = door_device(orc.VEL, True, slots=3)
    pl.set_max_num(S.REUSE_MAX_NUM)
    batch = pl.plan_batch(starts, goals)
    trajs = [pl.get_traj(q) for q in range(16)]
    assert [b["status"] for b in batch] == [c["status"] for c in ref]
    assert {(b["status"], b["n_expanded"] > 0) for b in batch} == {(0, True), (0, False), (1, True), (3, True)}
    one_pl = door_device(orc.VEL, True)
    one_pl.set_max_num(S.REUSE_MAX_NUM)
    for q in range(16):
        one = one_pl.plan_batch(starts[q:q + 1], goals[q:q + 1])[0]
        for k in ("status", "cost", "n_expanded", "n_nodes", "expand_hash", "traj_len"):
            assert one[k] == batch[q][k] or (k == "cost" and math.isinf(one[k]) and math.isinf(batch[q][k])), (q, k)
        t1 = one_pl.get_traj()
        assert (t1 is None) == (trajs[q] is None)
        if t1 is not None:
            assert np.array_equal(t1["states"], trajs[q]["states"]) and np.array_equal(t1["actions"], trajs[q]["actions"])
    for q in range(0, 16, 4):
        c = ref[q]
        assert batch[q]["status"] == c["status"] and batch[q]["n_expanded"] == len(c["expanded"])
        assert batch[q]["expand_hash"] == K.expand_hash(c["expanded"])
        if c["status"] == 0 and c["traj"] is not None:
            assert batch[q]["cost"] == c["cost"]
            assert np.array_equal(trajs[q]["states"], c["traj"]["states"])


# ---- the index's cells, seen through the count of point tests
M64 = (1 << 64) - 1


def bucket_of(cell, mask):
    """cloud_bucket (mplx_cloud.h) restated: the three cell coordinates, as 64-bit two's complement, mixed and masked"""
    h = ((cell[0] & M64) * 0x9E3779B97F4A7C15 & M64) ^ ((cell[1] & M64) * 0xC2B2AE3D27D4EB4F & M64) ^ ((cell[2] & M64) * 0x165667B19E3779F9 & M64)
    h ^= h >> 31
    h = h * 0xBF58476D1CE4E5B9 & M64
    h ^= h >> 29
    return h & 0xFFFFFFFF & mask


def untouched_states(name, control):
    """the states of a scene none of whose primitives a point blocks: every ellipsoid of theirs is tested against all 27 cells in full"""
    sc = S.SCENES[name]
    states = S.build(name, control)[1]
    free = valid_of([S.checker(sc, control, []).get_succ(s) for s in states])
    return states[(free == valid_of(reference(name, control)[1])).all(axis=1)]


def expected_point_tests(name, control, states):
    """points the radius filter looks at for `states`: for every ellipsoid of every primitive that reaches the point test, the sizes of
    the buckets of the 27 cells around the cell floor(x_f / (1.0625 r_f)) of its float32 centre, M = next_pow2(n) buckets"""
    sc = S.SCENES[name]
    pts = S.build(name, control)[0]
    ck = reference(name, control)[0]
    mask = 1
    while mask < len(pts):
        mask <<= 1
    mask -= 1
    size = {}
    for p in pts:
        b = bucket_of([S.cell_of(x, sc["r"]) for x in p], mask)
        size[b] = size.get(b, 0) + 1
    total = 0
    for s13 in states:
        for i in range(len(ck.U)):
            moves, validated, box, n = stage(ck, s13, i)
            if not (moves and validated and all(box)):
                continue
            for d, _, _ in S.ellipsoids(ck, s13, i):
                c = [S.cell_of(x, sc["r"]) for x in d]
                total += sum(size.get(bucket_of((c[0] + i0, c[1] + i1, c[2] + i2), mask), 0) for i0 in (-1, 0, 1) for i1 in (-1, 0, 1) for i2 in (-1, 0, 1))
    return total


COUNTED = [("index_1", orc.ACC), ("index_3", orc.ACC), ("index_5", orc.ACC), ("index_8", orc.ACC), ("eq_m1e4", orc.ACC), ("eq_1e5", orc.ACC),
           ("farm1e4_r005", orc.VEL)]


def test_untouched_states_exist_at_negative_cell_indices():
    for name, control in COUNTED:
        st = untouched_states(name, control)
        print(name, len(st), expected_point_tests(name, control, st))
        assert len(st) >= 4
    assert sum((untouched_states(n, c)[:, 0:3] < -1.0).any(axis=1).sum() for n, c in COUNTED) >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", [pytest.param(n, c, id=n) for n, c in COUNTED])
def test_point_test_count_of_untouched_states_equals_the_restated_index(name, control):
    """What get_succ returns cannot tell the index's cell function from another monotone one (both stay conservative); the number of
    points the radius filter looked at can: it is the content of the 27 buckets around every ellipsoid, no more (a state none of whose
    primitives is blocked has no early exit)"""
    st = untouched_states(name, control)
    pl = device(S.SCENES[name], control, S.build(name, control)[0])
    pl.get_succ_batch(st)
    assert pl.last_point_tests() == expected_point_tests(name, control, st)
