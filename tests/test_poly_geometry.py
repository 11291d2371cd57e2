"""The 2-D moving-obstacle planner swept across the fast paths of its collision test (switches P1..P9 of
mpl_ros_amd/csrc/mplx_poly_dev.h; DESIGN.md "The 2-D moving-obstacle sweep"), on the scenes of tests/poly_scenes.py.

CPU: (needs oracle/_ref) the checker tests/poly_checker.CheckerWorld equals the compiled reference on every scene, get_succ
and one plan, bit for bit; and every scene shows the regime it is named for, restated from the scene data and the checker
alone (never the library).  -m gpu: get_succ_batch, plan_batch (every kernel shape the host picks), PolyLpa and PolyLpaFleet
against the checker / the compiled reference's LPA*, bit for bit.  No scene is skipped or filtered on the GPU side; the
minimum counts of finite / infinite costs and of plans found (COUNTS) are what the checker gives with the seed fixed."""
import numpy as np
import pytest

from mpl_ros_amd import poly_map as pm
from oracle import refpoly
from tests import poly_checker as pc
from tests import poly_scenes as ps
from tests.poly_compare import compare_get_succ, compare_plans

needs_ref = pytest.mark.skipif(not refpoly.available(), reason="oracle/_ref/libpolymap_ref.so (Dim = 2; Dim = 3 is libpolymap3_ref.so) not built (make -C oracle ref)")
ACC, JRK, VEL, SNP = pm.ACC, pm.JRK, pm.VEL, pm.SNP
NAMES = list(ps.SCENES)
CTRL_NAME = {ACC: "acc", JRK: "jrk", VEL: "vel", SNP: "snp"}


def _cases(tag, controls):
    return [pytest.param(n, c, id=f"{n}-{CTRL_NAME[c]}") for c in controls for n in NAMES if tag is None or tag in ps.get(n).tags]


SUCC_CASES = _cases(None, [ACC]) + _cases("jrk", [JRK]) + _cases("velsnp", [VEL, SNP])
PLAN_CASES = _cases(None, [ACC]) + _cases("jrk", [JRK])
SHAPE_NAMES = [n for n in NAMES if "shapes" in ps.get(n).tags]
LPA_WORLD = {"count_edge": 2, "seg_span": 0, "hp_counts": 2, "deep": 0}  # (65 obstacles, dt / 10 segments, the 17-gon, the deep plan)

# (finite-cost successors, infinite-cost successors, plans found) the checker gives on the scene's states / plans, seed fixed
COUNTS = {
    ("count_small", ACC): (416, 196, 2),
    ("count_edge", ACC): (832, 452, 3),
    ("count_100", ACC): (446, 517, 1),
    ("seg_span", ACC): (1271, 340, 2),
    ("lds_limits", ACC): (1033, 518, 3),
    ("hp_counts", ACC): (1045, 572, 2),
    ("nu_1", ACC): (60, 5, 1),
    ("nu_25", ACC): (1347, 373, 1),
    ("nu_31", ACC): (1640, 440, 1),
    ("nu_32", ACC): (1511, 602, 1),
    ("nu_32_full", ACC): (1432, 715, 1),
    ("items_edge", ACC): (443, 677, 1),
    ("fast_off", ACC): (784, 470, 2),
    ("fast_mixed", ACC): (773, 292, 1),
    ("presence", ACC): (1186, 227, 2),
    ("linear", ACC): (823, 341, 2),
    ("time_dt025", ACC): (952, 158, 1),
    ("time_dt1", ACC): (729, 321, 1),
    ("time_dt03", ACC): (342, 367, 2),
    ("deep", ACC): (594, 126, 1),
    ("tags", ACC): (668, 391, 8),
    ("knife", ACC): (546, 327, 1),
    ("count_edge", JRK): (609, 294, 2),
    ("seg_span", JRK): (956, 249, 1),
    ("hp_counts", JRK): (762, 409, 2),
    ("fast_mixed", JRK): (538, 224, 1),
    ("count_100", VEL): (433, 505, 0),
    ("seg_span", VEL): (1258, 353, 0),
    ("linear", VEL): (810, 354, 0),
    ("knife", VEL): (574, 314, 0),
    ("count_100", SNP): (312, 408, 0),
    ("seg_span", SNP): (972, 236, 0),
    ("linear", SNP): (589, 282, 0),
    ("knife", SNP): (448, 240, 0),
}
# deepest expanded time level of the first plan (the checker's node(i)[0][8]), scenes that are there for it
LEVELS = {"deep": 120}


def scene(name, control=ACC):
    S = ps.get(name)
    return S if control == S.control else ps.with_control(S, control)


class Memo:
    """A checker world that computes every get_succ and every plan once per process (the same reference serves the regime
    test, the get_succ / plan comparisons and every kernel shape); node() answers for the path of the last plan() asked for."""

    def __init__(self, chk):
        self.chk, self.succ, self.plans, self.cur = chk, {}, {}, None

    def get_succ(self, s):
        key = np.ascontiguousarray(s, dtype=np.float64).tobytes()
        if key not in self.succ:
            self.succ[key] = self.chk.get_succ(s)
        return self.succ[key]

    def plan(self, start, goal, **kw):
        kw = dict(dict(eps=1.0, tol_pos=0.5, max_expand=-1, heur_ignore_dynamics=True), **kw)  # (one key however the defaults are spelt)
        key = (np.ascontiguousarray(start, dtype=np.float64).tobytes(), np.ascontiguousarray(goal, dtype=np.float64).tobytes(), tuple(sorted(kw.items())))
        if key not in self.plans:
            r = self.chk.plan(start, goal, **kw)
            nodes = {int(i): self.chk.node(int(i)) for i in r["node_ids"]}
            r["max_t"] = max((self.chk.node(int(i))[0][-1] for i in r["expanded"]), default=start[-1])
            self.plans[key] = (r, nodes)
        r, self.cur = self.plans[key]
        return r

    def node(self, i):
        return self.cur[int(i)]


_memo = {}


def checkers(S):
    key = (S.name, S.control)
    if key not in _memo:
        _memo[key] = [Memo(pc.CheckerWorld(W, S.control, S.U, **S.env)) for W in S.worlds]
    return _memo[key]


def plan_args(S, heur_ignore_dynamics=True):
    kw = dict(S.plans[0]["kw"], heur_ignore_dynamics=heur_ignore_dynamics)
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


# ---------------------------------------------------------------- CPU: the checker is the compiled reference on these scenes
def _same_succ(a, b):
    (sa, ca, aa), (sb, cb, ab) = a, b
    assert np.array_equal(aa, ab)
    assert np.array_equal(sa, sb) and np.array_equal(np.signbit(sa), np.signbit(sb))  # bit-exact f64, the signs of zero too
    assert all(x == y or (np.isinf(x) and np.isinf(y)) for x, y in zip(ca, cb))


@needs_ref
@pytest.mark.parametrize("name,control", SUCC_CASES)
def test_checker_equals_the_compiled_reference_get_succ(name, control):
    S = scene(name, control)
    chks = checkers(S)
    refs = [refpoly.RefWorld(W, S.control, S.U, **S.env) for W in S.worlds]
    for w, s in zip(S.world_of, S.states):
        _same_succ(chks[w].get_succ(s), refs[w].get_succ(s))


HEUR_NAMES = [n for n in NAMES if "heur" in ps.get(n).tags]
REF_PLAN_CASES = [pytest.param(*p.values, True, id=p.id) for p in PLAN_CASES] + [pytest.param(n, ACC, False, id=f"{n}-acc-dynamics") for n in HEUR_NAMES]


@needs_ref
@pytest.mark.parametrize("name,control,heur_ignore_dynamics", REF_PLAN_CASES)
def test_checker_equals_the_compiled_reference_plan(name, control, heur_ignore_dynamics):
    """one plan per scene (the first one the checker finds), `_same_plan` of test_poly_map3d.py; with the dynamics-aware heuristic
    too on the scenes the GPU side runs with it"""
    from tests.test_poly_map3d import _same_plan
    S = scene(name, control)
    chks = checkers(S)
    found = [p for p in S.plans if chks[p["world"]].plan(p["start"], p["goal"], **dict(p["kw"], heur_ignore_dynamics=heur_ignore_dynamics))["status"] == 0]
    assert found  # (a plan that is found: cost, actions, node ids and path states are compared, not only the expansion order)
    p = found[0]
    chk = chks[p["world"]]
    ref = refpoly.RefWorld(S.worlds[p["world"]], S.control, S.U, **S.env)
    kw = dict(p["kw"], heur_ignore_dynamics=heur_ignore_dynamics)
    a, b = ref.plan(p["start"], p["goal"], **kw), chk.plan(p["start"], p["goal"], **kw)
    assert a["status"] == 0
    _same_plan(a, b, ref, chk, [0, 1, 2, 3, 4, 5, 8] if control == JRK else [0, 1, 2, 3, 8])


# ---------------------------------------------------------------- CPU: the regimes, from the scene data and the checker alone
POLY_MAX_OBS, POLY_SLOTS, POLY_LDS_HPS, POLY_LDS_SEGS, POLY_CACHE_LEVELS, ICAP = 64, 3, 256, 256, 64, 1022


def obstacles(W):
    return W.static + W.linear + W.nonlinear


def hp_sum(W):
    return sum(len(o.poly) for o in obstacles(W))


def seg_sum(W):
    return sum(len(o.segs) for o in W.nonlinear)


def staged(W):
    """P3: the world is held in LDS"""
    return len(obstacles(W)) <= POLY_MAX_OBS and hp_sum(W) <= POLY_LDS_HPS and seg_sum(W) <= POLY_LDS_SEGS


def overlap(o, traj_t, prT):
    """P2: the segments collide()'s loop visits for a primitive of duration prT that starts at trajectory time traj_t"""
    T, start = 0.0, -1
    for i, sg in enumerate(o.segs):
        if traj_t >= T and traj_t < T + sg[12]:
            start = i
            break
        T += sg[12]
    if start < 0:
        return 0
    n = 0
    for sg in o.segs[start:]:
        if (0.0 if T - traj_t < 0 else T - traj_t) > prT:
            break
        n += 1
        T += sg[12]
    return n


def fourth_counts(o, traj_t, prT):
    """P2: a segment beyond the POLY_SLOTS-th of the span whose roots collide() can accept (it >= t_residual and it + T <= T + T_seg)"""
    T, start = 0.0, -1
    for i, sg in enumerate(o.segs):
        if traj_t >= T and traj_t < T + sg[12]:
            start = i
            break
        T += sg[12]
    if start < 0:
        return False
    for k, sg in enumerate(o.segs[start:]):
        res = 0.0 if T - traj_t < 0 else T - traj_t
        if res > prT:
            break
        if k >= POLY_SLOTS and res <= sg[12]:
            return True
        T += sg[12]
    return False


def is_fast(o):
    """P5: every segment VEL / ACC with T > 0 and +0.0 leading coefficients"""
    lead = o.segs[:, [0, 1, 2, 6, 7, 8]]
    return int(bool(np.all(o.segs[:, 12] > 0) and np.all(lead == 0.0) and not np.any(np.signbit(lead))))


def high_degree(W):
    return any(np.any(o.segs[:, [0, 1, 2, 6, 7, 8]] != 0.0) for o in W.nonlinear)


def spans(S):
    """overlap counts over every (trajectory, state) of the scene"""
    out = set()
    for w, s in zip(S.world_of, S.states):
        W = S.worlds[w]
        for o in W.nonlinear:
            out.add(overlap(o, (s[8] - W.start_t) + o.start_t, S.dt))
    return out


def unbounded(poly):
    """P6: fewer than three hyperplanes, or normals that leave a half turn uncovered"""
    ang = np.sort(np.arctan2(poly[:, 3], poly[:, 2]))
    gaps = np.diff(np.concatenate([ang, ang[:1] + 2 * np.pi]))
    return len(poly) < 3 or gaps.max() >= np.pi - 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_scene_shows_its_regime(name):
    S = ps.get(name)
    E = dict(S.expect)
    chks = checkers(S)
    world_of, starts, goals, kw = plan_args(S)
    # both outcomes, and the plans the scene promises -- for every control kind the GPU side runs on it
    for n, c in [p.values for p in SUCC_CASES if p.values[0] == name]:
        got = checker_counts(scene(n, c))
        assert got == COUNTS[(name, c)], (name, c, got)
        assert got[0] > 0 and got[1] > 0
    assert all(v[2] >= 1 for (n, c), v in COUNTS.items() if n == name and c in (ACC, JRK))  # ACC and JRK: a plan is found, its path compared
    n_obs = [len(obstacles(W)) for W in S.worlds]
    if "n_obs" in E:
        assert n_obs == E.pop("n_obs")
    if "n_u" in E:
        assert S.n_u == E.pop("n_u")
    if "pairs" in E:
        pairs = E.pop("pairs")
        assert all(S.n_u * n == pairs for n in n_obs)
    if "hp_sum" in E:
        assert [hp_sum(W) for W in S.worlds] == E.pop("hp_sum")
        assert [staged(W) for W in S.worlds][:2] == [True, False] and all(n <= POLY_MAX_OBS for n in n_obs)
    if "seg_sum" in E:
        assert [seg_sum(W) for W in S.worlds][2:] == E.pop("seg_sum")[2:]
        assert [staged(W) for W in S.worlds][2:] == [True, False]
    if "overlaps" in E:
        got = spans(S)
        assert E.pop("overlaps") <= got and POLY_SLOTS in got and any(k > POLY_SLOTS for k in got), got  # exactly 3 slots, and mode 4
        assert max(len(o.segs) for o in S.worlds[0].nonlinear) == E.pop("max_n_seg") >= 40
        assert {o.start_t for o in S.worlds[0].nonlinear} == {0.0, 0.3}
        # a fourth overlapped segment that can contribute: t_residual of that segment within its own duration, for some state
        assert E.pop("long_fourth") and any(fourth_counts(o, (s[8] - S.worlds[0].start_t) + o.start_t, S.dt) for o in S.worlds[0].nonlinear for s in S.states)
    if "hp_max" in E:
        assert [max(len(o.poly) for o in obstacles(W)) for W in S.worlds] == E.pop("hp_max")  # <= 15: the dense list; 16, 40: rectangular
        assert {len(o.poly) for W in S.worlds for o in obstacles(W)} == E.pop("n_hp")
        assert sum(int(unbounded(o.poly)) for W in S.worlds for o in obstacles(W)) == E.pop("unbounded")
        off = S.worlds[0].static[2].poly  # the pentagon whose reference point (the origin of its frame) lies outside it
        assert np.any(off[:, 2] * (0.0 - off[:, 0]) + off[:, 3] * (0.0 - off[:, 1]) > 1e-10)
        dup = S.worlds[0].linear[1].poly
        assert np.array_equal(dup[1], dup[3])
    if "items" in E:
        # mode 2 only (never pruned): items = valid primitives x sum of hyperplanes
        assert all(not W.static and not W.nonlinear for W in S.worlds) and E.pop("all_valid")
        for w, s in zip(S.world_of, S.states):
            assert len(chks[w].get_succ(s)[2]) == S.n_u
        items = [S.n_u * hp_sum(W) for W in S.worlds]
        assert items == E.pop("items") and items[0] == ICAP and items[1] > ICAP and max(len(o.poly) for W in S.worlds for o in obstacles(W)) <= 15
    if "fast" in E:
        assert [is_fast(o) for o in S.worlds[0].nonlinear] == E.pop("fast")
        assert high_degree(S.worlds[0]) == E.pop("high_degree")
        assert staged(S.worlds[0])  # (the shortcuts need cum: the staged world)
    if "traj_times" in E:
        W = S.worlds[0]
        assert {(s[8] - W.start_t) + W.nonlinear[0].start_t for s in S.states[:128]} == E.pop("traj_times")
        assert float(np.sum(W.nonlinear[0].segs[:, 12])) == E.pop("total_t")
        assert [(o.disappear_front, o.disappear_back) for o in W.nonlinear] == [(False, False), (True, False), (False, True), (True, True)]
    if "cov_v" in E:
        L = S.worlds[0].linear
        assert {o.cov_v for o in L} == E.pop("cov_v") and sum(int(not np.any(o.v)) for o in L) == E.pop("v_zero")
        c = chks[0]
        gone = {float(s[8]): bool(np.all(np.isfinite(c.get_succ(s)[1]))) for s in S.states[:12]}
        assert not gone[0.0] and not gone[2.0] and gone[2.5] and gone[3.5]  # the shrinking square blocks its centre until t = 2, then is gone
    if "dt" in E:
        assert S.dt == E.pop("dt") and S.worlds[0].start_t == E.pop("start_t")
        assert np.any(S.states[:, 8] < S.worlds[0].start_t)
        if "cache_level" in E:  # P7: no plan of the scene ever has t_rel / dt in [0, 64)
            assert not E.pop("cache_level")
            for p in S.plans:
                lv = (p["start"][8] - S.worlds[0].start_t) / S.dt
                assert lv < -p["kw"]["max_expand"] or lv >= POLY_CACHE_LEVELS
    if "min_levels" in E:
        p = S.plans[0]
        r = chks[p["world"]].plan(p["start"], p["goal"], **kw)
        levels = int(round((r["max_t"] - p["start"][8]) / S.dt))
        assert levels == LEVELS[name] and levels >= E.pop("min_levels") > POLY_CACHE_LEVELS and r["status"] == 0
    if "equal_start_t" in E:
        assert E.pop("equal_start_t") and len({W.start_t for W in S.worlds}) == 1 and len({p["start"][8] for p in S.plans}) == 1
        assert len(S.plans) > len(S.worlds)
    if "prune_edge" in E:
        rx = E.pop("prune_edge")
        st = S.worlds[0].static
        assert abs(st[2].p[0] - 1.0) < rx < abs(st[2].p[0] - 1.0) + 2e-9 and abs(st[3].p[1] - 3.0) > rx > abs(st[3].p[1] - 3.0) - 2e-9
    assert not E, E


# ---------------------------------------------------------------- GPU
def make_team(S, worlds=None, slots=16):
    team = pm.PolyTeam()
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
    R, n_ok = compare_plans(make_team(S), checkers(S), world_of, starts, goals, compare_acc=control == JRK, **kw)
    assert n_ok == COUNTS[(name, control)][2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", HEUR_NAMES)
def test_plan_batch_matches_the_checker_with_the_dynamics_aware_heuristic(name):
    S = ps.get(name)
    world_of, starts, goals, kw = plan_args(S, heur_ignore_dynamics=False)
    R, n_ok = compare_plans(make_team(S), checkers(S), world_of, starts, goals, **kw)
    assert n_ok >= 1


def _fields(team, R):
    return [(r.status, r.n_expanded, r.n_nodes, r.n_edges, r.cost, r.expand_hash, r.traj_len) + tuple(team.traj(k)[0].tolist()) for k, r in enumerate(R)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_every_kernel_shape_gives_the_checkers_plans(name):
    """helpers off, 3 per leader and automatic (64-lane leaders + 256-lane helper workgroups), then more queries than slots
    (256-lane workgroups that take several queries each, the per-level cache re-used under another query's tags): the same
    plans as the checker's, field for field the same as each other"""
    S = ps.get(name)
    world_of, starts, goals, kw = plan_args(S)
    world_of, starts, goals = world_of * 2, np.concatenate([starts, starts]), np.concatenate([goals, goals])  # (at least two queries)
    chks = checkers(S)
    team = make_team(S)
    runs = {}
    for h in (0, 3, -1):
        team.set_helpers(h)
        R, _ = compare_plans(team, chks, world_of, starts, goals, **kw)
        runs[h] = _fields(team, R)
        if S.n_u <= 31:
            assert team.last_helpers() == (h if h >= 0 else 4), (h, team.last_helpers())
        else:
            assert team.last_helpers() == 0  # P8: the masks hold 31 hit bits
    few = make_team(S, slots=max(1, len(world_of) // 3))
    R, _ = compare_plans(few, chks, world_of, starts, goals, **kw)
    assert few.last_helpers() == 0
    runs["few"] = _fields(few, R)
    assert runs[0] == runs[3] == runs[-1] == runs["few"]


@pytest.mark.gpu
def test_set_worlds_again_with_another_obstacle_count_then_plan():
    """one handle: 10-obstacle worlds, then worlds of 63..65 obstacles, then the first again -- nothing of an earlier commit
    (staged world, cache entries, obstacle counts) survives into the next plans"""
    A, B = ps.get("tags"), ps.get("count_edge")
    assert A.env == B.env and np.array_equal(A.U, B.U)
    team = make_team(A)
    for S in (A, B, A):
        team.set_worlds(S.worlds)
        world_of, starts, goals, kw = plan_args(S)
        R, n_ok = compare_plans(team, checkers(S), world_of, starts, goals, **kw)
        assert n_ok == COUNTS[(S.name, ACC)][2]


# ---------------------------------------------------------------- GPU: LPA*
def moved(W, tick):
    """the world one tick (0.5 s) later: linear obstacles where they have moved to, the planner's start time advanced
    (poly_map_replanner_node.cpp:123-131), static obstacles pushed aside, trajectories further along"""
    V = pm.PolyWorld(W.ori, W.dim, start_t=W.start_t + tick)
    V.static = [pm.StaticObstacle(o.poly, o.p + np.array([0.4, -0.3])) for o in W.static]
    V.linear = [pm.LinearObstacle(o.poly, o.p + o.v * tick + np.array([-0.3, 0.4]), o.v, o.cov_v) for o in W.linear]
    # (t_rel falls by `tick` with the start time: a trajectory one tick further along starts 2 ticks later in the planner's time)
    V.nonlinear = [pm.NonlinearObstacle(o.poly, o.segs, o.start_t + 2 * tick, o.disappear_front, o.disappear_back) for o in W.nonlinear]
    return V


def lpa_setup(name):
    S = ps.get(name)
    p = [q for q in S.plans if q["world"] == LPA_WORLD[name]][0]
    W = S.worlds[p["world"]]
    kw = dict(eps=p["kw"].get("eps", 1.0), max_expand=p["kw"]["max_expand"])
    return S, W, moved(W, 0.5), p["start"], p["goal"], kw


@pytest.mark.gpu
@needs_ref
@pytest.mark.parametrize("name", list(LPA_WORLD))
def test_poly_lpa_plans_and_repairs_like_the_compiled_reference(name):
    """plan, set_worlds with the obstacles moved, update_nodes, plan again: every state's g / rhs / h / flags, every entry with
    its blocked bit, the entries updateNodes reports, expansion order, cost and trajectory (`compare` of test_poly_lpa.py)"""
    from tests.test_poly_lpa import compare
    S, W, W2, start, goal, kw = lpa_setup(name)
    Lo = refpoly.RefWorld(W, S.control, S.U, **S.env)
    Lo.lpa_reset()
    team = make_team(S, [W], slots=1)
    l = team.lpa()
    l.set_capacity(1 << 18, 1 << 21, 1 << 20)
    ro = Lo.lpa_plan(start, goal, **kw)
    compare(Lo, l, ro, l.plan(start, goal, **kw), S.control)
    assert ro["status"] == 0
    Lo.reload(W2)
    team.set_worlds([W2])
    uo, ud = Lo.lpa_update_nodes(), l.update_nodes()
    assert ud == uo, (ud[:2], uo[:2])
    assert uo[0] + uo[1] > 0  # (the move changes stored collision outcomes: a repair, not a no-op)
    ro = Lo.lpa_plan(start, goal, **kw)
    compare(Lo, l, ro, l.plan(start, goal, **kw), S.control)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LPA_WORLD))
def test_poly_lpa_fleet_members_are_the_single_handles(name):
    """four members (two on the world, two on the moved world, goals apart) through plan / set_worlds / update_nodes / plan, in one
    launch each, against four single PolyLpa handles given the same calls: bit for bit"""
    from tests.test_plpa_fleet import same_snapshots, snapshot
    S, W, W2, start, goal, kw = lpa_setup(name)
    W3 = moved(W2, 0.5)
    world_of = [0, 1, 0, 1]
    starts = np.array([start] * 4)
    goals = np.array([goal] * 4)
    goals[2:, 1] -= 0.7
    ta, tb = make_team(S, [W, W2], slots=4), make_team(S, [W, W2], slots=4)
    fleet = ta.lpa_fleet(world_of)
    fleet.set_capacity(1 << 18, 1 << 21, 1 << 20)
    singles = [pm.PolyLpa(tb, w) for w in world_of]
    for l in singles:
        l.set_capacity(1 << 18, 1 << 21, 1 << 20)

    def plan_and_compare(where):
        fleet.plan(starts, goals, **kw)
        for i, l in enumerate(singles):
            l.plan(starts[i], goals[i], **kw)
            assert fleet.member(i).result.as_dict() == l.result.as_dict(), (where, i)
            same_snapshots(snapshot(fleet.member(i)), snapshot(l), (where, i))

    plan_and_compare("fresh")
    ta.set_worlds([W2, W3])
    tb.set_worlds([W2, W3])
    assert fleet.update_nodes() == [l.update_nodes() for l in singles]
    plan_and_compare("repair")
