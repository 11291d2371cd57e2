"""The 3-D moving-obstacle planner (mplx_poly3_*, mpl_ros_amd/csrc/mplx_poly3.h and mplx_poly3.hip) swept across the code paths
of its kernels and of its host code (DESIGN.md "The 3-D moving-obstacle sweep"), on the scenes of tests/poly3_scenes.py.

CPU: (needs oracle/_ref/libpolymap3_ref.so) the checker tests/poly_checker.CheckerWorld equals the reference's own headers
compiled at Dim = 3 on every scene -- get_succ in every control kind the GPU side runs, one found plan per control, isInside and
isFree(pt, t) around the six faces -- bit for bit; every scene shows the regime it is named for, restated from the scene data
and the checker alone (never the library); COUNTS is what the checker gives with the seed fixed.  -m gpu: get_succ_batch,
plan_batch, nodes(), batch identity and handle reuse against the checker, bit for bit.  No scene is skipped or filtered on
the GPU side."""
import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd import poly_map3d as p3
from oracle import refpoly
from tests import poly3_scenes as ps
from tests import poly_checker as pc
from tests.poly_compare import compare_get_succ, compare_plans, path_cols, same_plan, same_succ
from tests.test_poly_geometry import Memo

needs_ref = pytest.mark.skipif(not refpoly.available(3), reason="oracle/_ref/libpolymap3_ref.so (Dim = 3; Dim = 2 is libpolymap_ref.so) not built (make -C oracle ref)")
ACC, JRK, VEL, SNP = ps.ACC, ps.JRK, ps.VEL, ps.SNP
NAMES = list(ps.SCENES)
CTRL_NAME = {ACC: "acc", JRK: "jrk", VEL: "vel", SNP: "snp"}
POLY3_MAX_U = 32


def _cases(tag, controls):
    return [pytest.param(n, c, id=f"{n}-{CTRL_NAME[c]}") for c in controls for n in NAMES if tag is None or tag in ps.get(n).tags]


SUCC_CASES = _cases(None, [ACC]) + _cases("jrk", [JRK]) + _cases("velsnp", [VEL, SNP])
PLAN_CASES = _cases(None, [ACC]) + _cases("jrk", [JRK])
HEUR_NAMES = [n for n in NAMES if "heur" in ps.get(n).tags]
TOLVEL_NAMES = [n for n in NAMES if "tolvel" in ps.get(n).tags]
assert sum(1 for p in SUCC_CASES if p.values[1] == SNP) >= 4

# (finite-cost successors, infinite-cost successors, plans found) the checker gives on the scene's states / plans, seed fixed
COUNTS = {
    ("pairs_one_pass", ACC): (2871, 627, 2),
    ("pairs_strided", ACC): (4109, 742, 2),
    ("obs_300", ACC): (2119, 1652, 2),
    ("obs_0_1", ACC): (2028, 390, 2),
    ("uneven_batch", ACC): (3906, 954, 3),
    ("nu_1", ACC): (158, 19, 1),
    ("nu_7", ACC): (1073, 118, 2),
    ("nu_32", ACC): (4850, 720, 2),
    ("box_far", ACC): (3475, 578, 2),
    ("box_thin", ACC): (1349, 397, 2),
    ("time_dt025", ACC): (4060, 413, 2),
    ("time_dt03", ACC): (3913, 587, 2),
    ("time_dt1", ACC): (3106, 370, 2),
    ("deep", ACC): (888, 217, 2),
    ("degree_z3", ACC): (2580, 324, 1),
    ("degree_4_5", ACC): (2509, 818, 1),
    ("jerk_zero", ACC): (3079, 917, 2),
    ("seg_short", ACC): (2336, 805, 2),
    ("presence", ACC): (3855, 627, 2),
    ("overrun", ACC): (3621, 591, 3),
    ("shapes", ACC): (3058, 1220, 2),
    ("limits_off", ACC): (2131, 479, 2),
    ("pairs_strided", JRK): (4141, 746, 2),
    ("nu_7", JRK): (1051, 105, 2),
    ("box_far", JRK): (3452, 517, 2),
    ("time_dt025", JRK): (4068, 387, 1),
    ("degree_4_5", JRK): (2511, 810, 2),
    ("jerk_zero", JRK): (3013, 956, 2),
    ("seg_short", JRK): (2322, 810, 2),
    ("overrun", JRK): (3601, 611, 2),
    ("limits_off", JRK): (2096, 496, 2),
    ("pairs_strided", VEL): (4084, 791, 0),
    ("box_far", VEL): (3395, 738, 0),
    ("degree_z3", VEL): (2605, 452, 0),
    ("seg_short", VEL): (2304, 855, 0),
    ("presence", VEL): (4020, 420, 0),
    ("shapes", VEL): (2875, 1370, 0),
    ("pairs_strided", SNP): (4131, 729, 0),
    ("box_far", SNP): (3564, 513, 0),
    ("degree_z3", SNP): (2652, 345, 0),
    ("seg_short", SNP): (2322, 810, 0),
    ("presence", SNP): (3627, 855, 0),
    ("shapes", SNP): (3057, 1272, 0),
}
# every scene but these gives at least 200 finite and 50 infinite successors and one found plan under ACC
SMALL = {"nu_1", "obs_0_1", "limits_off"}
# deepest expanded time level of the first plan (the checker's node(i)[0][12])
LEVELS = {"deep": 42}


def scene(name, control=ACC):
    S = ps.get(name)
    return S if control == S.control else ps.with_control(S, control)


_memo = {}


def checkers(S):
    """the scene's checker worlds, every get_succ and plan computed once per process (Memo of test_poly_geometry.py)"""
    key = (S.name, S.control, S.n_u, S.dt)
    if key not in _memo:
        _memo[key] = [Memo(pc.CheckerWorld(W, S.control, S.U, **S.env)) for W in S.worlds]
    return _memo[key]


def plan_args(S, **more):
    kw = dict(S.plans[0]["kw"], **more)
    assert all(p["kw"] == S.plans[0]["kw"] for p in S.plans)  # (one launch per scene: one set of plan parameters)
    return [p["world"] for p in S.plans], np.array([p["start"] for p in S.plans]), np.array([p["goal"] for p in S.plans]), kw


def checker_counts(S):
    chks = checkers(S)
    n_fin = n_inf = 0
    for w, s in zip(S.world_of, S.states):
        cost = chks[w].get_succ(s)[1]
        n_fin += int(np.isfinite(cost).sum()); n_inf += int(np.isinf(cost).sum())
    world_of, starts, goals, kw = plan_args(S)
    n_ok = sum(int(chks[w].plan(s, g, **kw)["status"] == 0) for w, s, g in zip(world_of, starts, goals)) if S.control in (ACC, JRK) else 0
    return n_fin, n_inf, n_ok


# ---------------------------------------------------------------- CPU: the checker is the compiled reference at Dim = 3
@needs_ref
@pytest.mark.parametrize("name,control", SUCC_CASES)
def test_checker_equals_the_compiled_reference_get_succ(name, control):
    S = scene(name, control)
    chks = checkers(S)
    refs = [refpoly.RefWorld3D(W, S.control, S.U, **S.env) for W in S.worlds]
    for w, s in zip(S.world_of, S.states):
        same_succ(chks[w].get_succ(s), refs[w].get_succ(s))


REF_PLAN_CASES = [pytest.param(*p.values, True, id=p.id) for p in PLAN_CASES] + \
    [pytest.param(n, ACC, False, id=f"{n}-acc-dynamics") for n in HEUR_NAMES]


@needs_ref
@pytest.mark.parametrize("name,control,heur_ignore_dynamics", REF_PLAN_CASES)
def test_checker_equals_the_compiled_reference_plan(name, control, heur_ignore_dynamics):
    """one plan per scene and control (the first one the checker finds): status, expansion order, node count, cost, actions, node
    ids and the path states over three axes"""
    S = scene(name, control)
    chks = checkers(S)
    found = [p for p in S.plans if chks[p["world"]].plan(p["start"], p["goal"], **dict(p["kw"], heur_ignore_dynamics=heur_ignore_dynamics))["status"] == 0]
    assert found  # (a plan that is found: cost, actions, node ids and path states are compared, not only the expansion order)
    p = found[0]
    chk = chks[p["world"]]
    ref = refpoly.RefWorld3D(S.worlds[p["world"]], S.control, S.U, **S.env)
    kw = dict(p["kw"], heur_ignore_dynamics=heur_ignore_dynamics)
    a, b = ref.plan(p["start"], p["goal"], **kw), chk.plan(p["start"], p["goal"], **kw)
    assert a["status"] == 0
    same_plan(a, b, ref, chk, path_cols(3, control == JRK))


@needs_ref
def test_is_inside_and_is_free_point_equal_the_compiled_reference_around_the_six_faces():
    """an off-origin, non-cubic box: points on each face, 1e-10 either side of it (Polyhedron::inside lets 1e-10 pass), the next
    double beyond that, and the eight corners; isFree(pt, t) at the same points and around the faces of an obstacle"""
    S = ps.get("box_far")
    W = S.worlds[0]
    chk, ref = pc.CheckerWorld(W, ACC, S.U, **S.env), refpoly.RefWorld3D(W, ACC, S.U, **S.env)
    lo, hi, mid = W.ori, W.ori + W.dim, W.ori + W.dim / 2
    pts = [np.where(np.array(c), hi, lo) for c in np.ndindex(2, 2, 2)]
    for ax in range(3):
        for edge, out in ((lo[ax], -1.0), (hi[ax], 1.0)):
            for d in (0.0, 1e-10, -1e-10, 2e-10, 1e-9):
                for base in (mid, lo + W.dim * (0.25, 0.75, 0.1)):
                    p = base.copy()
                    p[ax] = edge + out * d
                    pts.append(p)
                    p = p.copy()
                    p[ax] = np.nextafter(p[ax], out * np.inf)
                    pts.append(p)
    inside = [chk.is_inside(p) for p in pts]
    assert inside == [ref.is_inside(p) for p in pts]
    assert 0 < sum(inside) < len(pts)
    o = W.static[1]  # an obstacle's own faces: the hyperplane points moved to where the obstacle stands, and 1e-10 either side
    for hp in o.poly:
        for d in (0.0, 1e-10, -1e-10, 3e-10):
            pts.append(o.p + hp[0:3] + d * hp[3:6])
    pts += [ps.first_pos(q) for q in ps.obstacles(W)]
    free = [chk.is_free(p, t) for p in pts for t in (1.25, 1.75, 3.0)]
    assert free == [ref.is_free(p, t) for p in pts for t in (1.25, 1.75, 3.0)]
    assert 0 < sum(free) < len(free)


# ---------------------------------------------------------------- CPU: the regimes, from the scene data and the checker alone
def hp_sum(W):
    return sum(len(o.poly) for o in ps.obstacles(W))


def seg_sum(W):
    return sum(len(o.segs) for o in W.nonlinear)


def general(S, control):
    """the host's choice of the GEN kernels, restated: JRK / SNP primitives, or any segment with a non-zero coefficient above
    degree two"""
    return control in (JRK, SNP) or any(np.any(o.segs[:, [0, 1, 2, 6, 7, 8, 12, 13, 14]] != 0.0) for W in S.worlds for o in W.nonlinear)


def overlap(o, traj_t, prT):
    """the segments collide()'s loop visits for a primitive of duration prT that starts at trajectory time traj_t"""
    T, start = 0.0, -1
    for i, sg in enumerate(o.segs):
        if traj_t >= T and traj_t < T + sg[18]:
            start = i
            break
        T += sg[18]
    if start < 0:
        return 0
    n = 0
    for sg in o.segs[start:]:
        if (0.0 if T - traj_t < 0 else T - traj_t) > prT:
            break
        n += 1
        T += sg[18]
    return n


def start_hits(S, p):
    """(index of the expansion, finite-cost successors of later expansions) for every expanded node of plan p whose own position
    is not free at its own time -- isFree(start.pos, t) fails, every primitive out of it is blocked"""
    W = S.worlds[p["world"]]
    chk = pc.CheckerWorld(W, S.control, S.U, **S.env)
    r = chk.plan(p["start"], p["goal"], **p["kw"])
    nodes = [chk.node(int(i))[0] for i in r["expanded"]]
    fin = [int(np.isfinite(chk.get_succ(s)[1]).sum()) for s in nodes]
    return [(k, sum(fin[k + 1:])) for k, s in enumerate(nodes) if chk.is_inside(s[0:3]) and not chk.is_free(s[0:3], s[12])], r


@pytest.mark.parametrize("name", NAMES)
def test_scene_shows_its_regime(name):
    S = ps.get(name)
    E = dict(S.expect)
    chks = checkers(S)
    world_of, starts, goals, kw = plan_args(S)
    assert len(S.states) <= 200 and 2 <= len(S.plans) <= 4 and 120 <= kw["max_expand"] <= 600
    # both outcomes, and the plans the scene promises -- for every control kind the GPU side runs on it
    for n, c in [p.values for p in SUCC_CASES if p.values[0] == name]:
        got = checker_counts(scene(n, c))
        assert got == COUNTS[(name, c)], (name, c, got)
        assert got[0] > 0 and got[1] > 0
    if name not in SMALL:
        fin, inf, ok = COUNTS[(name, ACC)]
        assert fin >= 200 and inf >= 50 and ok >= 1
    assert all(v[2] >= 1 for (n, c), v in COUNTS.items() if n == name and c == JRK)  # JRK: a plan is found, its path compared
    n_obs = [len(ps.obstacles(W)) for W in S.worlds]
    assert all(len(o.segs) > 0 and np.all(o.segs[:, 18] >= 0) for W in S.worlds for o in W.nonlinear)  # (what the reference leaves undefined stays out)
    assert general(S, ACC) == bool(E.pop("gen_acc", False)) and general(S, JRK) and general(S, SNP)
    if "n_obs" in E:
        assert n_obs == E.pop("n_obs")
    if "n_u" in E:
        assert S.n_u == E.pop("n_u") <= POLY3_MAX_U
    if "pairs" in E:
        pairs = E.pop("pairs")
        assert [S.n_u * n for n in n_obs] == pairs
        if name == "pairs_one_pass":
            assert ps.BLOCK - S.n_u < pairs[0] <= ps.BLOCK  # one more obstacle and a lane takes a second trip
        if name in ("pairs_strided", "nu_32"):
            # a second trip, and it lands in another primitive: (e + 256) / n_obs != e / n_obs for every lane that takes one
            assert all(ps.BLOCK < q < 2 * ps.BLOCK and n < ps.BLOCK for q, n in zip(pairs, n_obs))
    if "late_start_hit" in E:
        # the start-point loop strides: states whose position only an obstacle beyond the 256th covers
        W = S.worlds[0]
        head = p3.PolyWorld3D(W.ori, W.dim, W.start_t)
        obs = ps.obstacles(W)[:ps.BLOCK]
        head.static, head.linear, head.nonlinear = [o for o in obs if o in W.static], [o for o in obs if o in W.linear], [o for o in obs if o in W.nonlinear]
        first = pc.CheckerWorld(head, S.control, S.U, **S.env)
        late = [s for s in S.states if first.is_free(s[0:3], s[12]) and not chks[0].chk.is_free(s[0:3], s[12])]
        assert E.pop("late_start_hit") and n_obs[0] > ps.BLOCK and len(late) >= 10
        assert all(np.all(np.isinf(chks[0].get_succ(s)[1])) and len(chks[0].get_succ(s)[1]) > 0 for s in late)
    if "unsorted" in E:
        assert E.pop("unsorted") and np.any(np.diff(S.world_of) < 0) and np.any(np.diff(world_of) < 0)
        assert len({hp_sum(W) for W in S.worlds}) == len(S.worlds) and len({seg_sum(W) for W in S.worlds}) == len(S.worlds)
        assert set(S.world_of.tolist()) == set(range(len(S.worlds))) == set(world_of)
    if "ori" in E:
        W = S.worlds[0]
        assert tuple(W.ori) == E.pop("ori") and tuple(W.dim) == E.pop("dim") and W.start_t == E.pop("start_t")
        on = {(ax, side) for s in S.states for ax in range(3) for side, edge in enumerate((W.ori[ax], W.ori[ax] + W.dim[ax])) if s[ax] == edge}
        assert len(on) == E.pop("faces") == 6
    if "dim_z" in E:
        assert S.worlds[0].dim[2] == E.pop("dim_z") < 0.5 * max(abs(u[2]) for u in S.U) * S.dt ** 2  # a node at rest leaves with u_z = +-1, wherever it is
        emitted = sum(len(chks[w].get_succ(s)[2]) for w, s in zip(S.world_of, S.states))
        assert emitted < E.pop("leave_share") * S.n_u * len(S.states)
    if "dt" in E:
        assert S.dt == E.pop("dt") and S.worlds[0].start_t == E.pop("start_t")
        assert np.any(S.states[:, 12] < S.worlds[0].start_t)
        ties = [abs((p["start"][12] + k * S.dt) / 0.1 % 1.0 - 0.5) < 1e-9 for p in S.plans for k in range(1, 5)]
        assert any(ties) == (name == "time_dt025")  # the key round(t / 0.1) on a tie
    if "min_levels" in E:
        p = S.plans[0]
        r = chks[p["world"]].plan(p["start"], p["goal"], **kw)
        levels = int(round((r["max_t"] - p["start"][12]) / S.dt))
        assert levels == LEVELS[name] and levels >= E.pop("min_levels") and r["status"] == 0
    if "degree" in E:
        kind = E.pop("degree")
        segs = np.concatenate([o.segs for W in S.worlds for o in W.nonlinear]).reshape(-1, 19)
        c = segs[:, :18].reshape(-1, 3, 6)
        if kind == "z3":  # cubic on z and on z only
            assert np.all(c[:, :, 0:2] == 0) and np.all(c[:, 0:2, 2] == 0) and np.all(c[:, 2, 2] != 0)
        else:             # quintic segments and quartic ones
            assert np.any(np.all(c[:, :, 0] != 0, axis=1)) and np.any((c[:, 0, 0] == 0) & (c[:, 0, 1] != 0))
    if "jrk_built" in E:
        segs = np.concatenate([o.segs for o in S.worlds[0].nonlinear]).reshape(-1, 19)
        jerk = segs[:, [2, 8, 14]]
        assert E.pop("jrk_built") and np.all(jerk == 0.0) and np.any(np.signbit(jerk)) and np.any(segs[:, [3, 9, 15]] != 0.0)
    if "overlaps" in E:
        W = S.worlds[0]
        got = {overlap(o, (s[12] - W.start_t) + o.start_t, S.dt) for s in S.states for o in W.nonlinear}
        assert E.pop("overlaps") <= got, got
        assert {len(o.segs) for o in W.nonlinear} == E.pop("n_seg")
        assert sum(int(np.any(o.segs[:, 18] == 0.0)) for o in W.nonlinear) == E.pop("zero_T")
        assert all(np.all(o.segs[o.segs[:, 18] > 0, 18] == S.dt / 10) for o in W.nonlinear)
    if "traj_times" in E:
        W = S.worlds[0]
        assert {(s[12] - W.start_t) + W.nonlinear[0].start_t for s in S.states[:128]} == E.pop("traj_times")
        assert float(np.sum(W.nonlinear[0].segs[:, 18])) == E.pop("total_t")
        assert [(o.disappear_front, o.disappear_back) for o in W.nonlinear] == [(False, False), (True, False), (False, True), (True, True)]
    if "start_hit_mid_plan" in E:
        # a node expanded in the middle of a plan that an obstacle covers at that time, with finite-cost expansions after it
        hits = [start_hits(S, p) for p in S.plans]
        assert E.pop("start_hit_mid_plan") and any(any(k > 0 and after > 0 for k, after in h) and r["status"] == 0 for h, r in hits), [h for h, _ in hits]
        assert S.worlds[0].linear and any(o.disappear_front and o.start_t < 0 for o in S.worlds[0].nonlinear)
    if "n_hp" in E:
        W = S.worlds[0]
        assert {len(o.poly) for o in ps.obstacles(W)} == E.pop("n_hp")
        off = W.static[1].poly  # the shape whose reference point (the origin of its frame) lies outside it
        assert E.pop("outside_ref") and np.any(np.sum(off[:, 3:6] * (0.0 - off[:, 0:3]), axis=1) > 1e-10)
        assert sum(int(o.cov_v > 0) for o in W.linear) == E.pop("cov_pos") and sum(int(not np.any(o.v)) for o in W.linear) == E.pop("v_zero")
        tilted = [o for o in ps.obstacles(W) if len(o.poly) == 20]
        assert tilted and all(np.all(np.abs(o.poly[:, 3:6]) < 0.95) for o in tilted)
    if "limits" in E:
        assert not E.pop("limits") and S.env["v_max"] == S.env["a_max"] == S.env["j_max"] == -1.0
    assert not E, E


# ---------------------------------------------------------------- GPU
def make_team(S, worlds=None, slots=16):
    team = p3.PolyTeam3D()
    team.configure(S.control, S.U, **S.env)
    team.set_worlds(S.worlds if worlds is None else worlds)
    team.set_capacity(slots, 1 << 20, 1 << 22, 1 << 21)
    return team


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", SUCC_CASES)
def test_get_succ_batch_matches_the_checker(name, control):
    S = scene(name, control)
    n_fin, n_inf = compare_get_succ(make_team(S), S.worlds, checkers(S), S.world_of, S.states, S.n_u, signs=True)
    assert (n_fin, n_inf) == COUNTS[(name, control)][:2]


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", PLAN_CASES)
def test_plan_batch_matches_the_checker(name, control):
    S = scene(name, control)
    world_of, starts, goals, kw = plan_args(S)
    R, n_ok = compare_plans(make_team(S), checkers(S), world_of, starts, goals, compare_acc=control == JRK, dim=3, **kw)
    assert n_ok == COUNTS[(name, control)][2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", HEUR_NAMES)
def test_plan_batch_matches_the_checker_with_the_dynamics_aware_heuristic(name):
    S = ps.get(name)
    world_of, starts, goals, kw = plan_args(S, heur_ignore_dynamics=False)
    R, n_ok = compare_plans(make_team(S), checkers(S), world_of, starts, goals, dim=3, **kw)
    assert n_ok >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", TOLVEL_NAMES)
def test_plan_batch_matches_the_checker_with_a_velocity_tolerance(name):
    """tol_vel = 0.5: the goal test bounds the velocity too (the second plan of these scenes carries a goal velocity)"""
    S = ps.get(name)
    assert any(np.any(p["goal"][3:6]) for p in S.plans)
    world_of, starts, goals, kw = plan_args(S, heur_ignore_dynamics=False, tol_vel=0.5)
    R, n_ok = compare_plans(make_team(S), checkers(S), world_of, starts, goals, dim=3, **kw)
    assert n_ok >= 1


@pytest.mark.gpu
def test_33_inputs_are_refused():
    team = p3.PolyTeam3D()
    U = np.zeros((POLY3_MAX_U + 1, 3))
    assert team.lib.mplx_poly3_config(team.h, ACC, POLY3_MAX_U + 1, U.ctypes.data, 0.5, 2.0, 1.5, 2.0, 10.0) == _capi.ERR_ARG
    assert team.lib.mplx_poly3_config(team.h, ACC, POLY3_MAX_U, U.ctypes.data, 0.5, 2.0, 1.5, 2.0, 10.0) == _capi.OK


@pytest.mark.gpu
@pytest.mark.parametrize("name,control", [("pairs_strided", ACC), ("nu_7", JRK)])
def test_result_nodes_match_the_checker_state_space(name, control):
    """every node of every plan: state (JRK: with the acceleration), g, and the closed / open flags of the checker's node(i)"""
    S = scene(name, control)
    world_of, starts, goals, kw = plan_args(S)
    team = make_team(S)
    R = team.plan_batch(world_of, starts, goals, **kw)
    cols = path_cols(3, control == JRK)
    for k, w in enumerate(world_of):
        chk = pc.CheckerWorld(S.worlds[w], S.control, S.U, **S.env)
        ref = chk.plan(starts[k], goals[k], **kw)
        assert R[k].status == ref["status"] and R[k].n_expanded == len(ref["expanded"])
        st, g, closed, opened = team.nodes(k)
        assert len(st) == ref["n_nodes"] == R[k].n_nodes > 50
        for i in range(len(st)):
            s, gi, _, cl, op = chk.node(i)
            assert np.array_equal(st[i][cols], s[cols]) and g[i] == gi, (k, i)
            assert bool(closed[i]) == bool(cl) and (bool(opened[i]) and not closed[i]) == (bool(op) and not cl), (k, i)


def _fields(team, k, r):
    return (r.status, r.cost, r.n_expanded, r.n_nodes, tuple(team.expanded_ids(k)), tuple(team.traj(k)[0]), tuple(team.traj(k)[1]))


@pytest.mark.gpu
def test_each_query_of_the_uneven_batch_plans_alone_as_it_does_in_the_batch():
    S = ps.get("uneven_batch")
    world_of, starts, goals, kw = plan_args(S)
    team = make_team(S)
    team.set_record(1 << 12)
    R = team.plan_batch(world_of, starts, goals, **kw)
    batch = [_fields(team, k, r) for k, r in enumerate(R)]
    assert len({b[2:4] for b in batch}) > 1  # (the worlds give different searches)
    for k in range(len(world_of)):
        r1 = team.plan_batch(world_of[k:k + 1], starts[k:k + 1], goals[k:k + 1], **kw)[0]
        assert _fields(team, 0, r1) == batch[k], k


def _compare_scene(team, S):
    n_fin, n_inf = compare_get_succ(team, S.worlds, checkers(S), S.world_of, S.states, S.n_u, signs=True)
    assert n_fin > 0 and n_inf > 0
    world_of, starts, goals, kw = plan_args(S)
    R, n_ok = compare_plans(team, checkers(S), world_of, starts, goals, compare_acc=S.control == JRK, dim=3, **kw)
    return n_fin, n_inf, n_ok


@pytest.mark.gpu
def test_one_handle_through_new_worlds_and_new_set_ups():
    """one PolyTeam3D: the quartic / quintic worlds (the general kernels), then quadratic-only worlds of another count (the host's
    high-degree mark must clear, the device arrays are replaced by ones of another size), then JRK with seven inputs and half the
    time step, then ACC with 27 again -- nothing of an earlier commit or set-up survives into the next answers"""
    A, B = ps.get("degree_4_5"), ps.get("uneven_batch")
    assert A.env == B.env and np.array_equal(A.U, B.U) and len(A.worlds) != len(B.worlds) and general(A, ACC) and not general(B, ACC)
    team = make_team(A)
    assert _compare_scene(team, A) == COUNTS[("degree_4_5", ACC)]
    team.set_worlds(B.worlds)
    assert _compare_scene(team, B) == COUNTS[("uneven_batch", ACC)]
    J = ps.with_control(B, JRK, U=ps.U7, dt=0.25)
    # (the 300-obstacle world under JRK costs the checker 40 ms per expansion: 60 states, and the plans of the other three worlds)
    J.states, J.world_of, J.plans = J.states[:60], J.world_of[:60], [p for p in J.plans if len(ps.obstacles(J.worlds[p["world"]])) < 100]
    assert len(J.plans) == 3 and set(J.world_of.tolist()) == {0, 1, 2, 3}
    team.configure(J.control, J.U, **J.env)
    assert _compare_scene(team, J)[2] >= 1
    team.configure(B.control, B.U, **B.env)
    assert _compare_scene(team, B) == COUNTS[("uneven_batch", ACC)]
