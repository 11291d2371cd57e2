"""Point-cloud searches guided by a prior trajectory (PlannerBase::setPriorTrajectory; the P-list of
mpl_ros_amd/csrc/mplx_cloud.h), against tests/cloud_prior_checker.py, bit for bit.

CPU: known answers of the checker itself.  GPU: the heuristic entry on the index boundaries of the table and every pairing of
control kinds; whole plans (prior shorter and longer than the plan, a start time, eps 0 / 1 / 2, a misleading prior that makes
states re-open, a table below and one above the LDS staging cap); batches with one prior per query and the life of a prior on
a handle.  One room of 12 x 6 x 2 m with a wall and a doorway, 180 points, nine control inputs, at most 300 expansions.
"""
import math

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd.ellipsoid import ACC, JRK, SNP, VEL, EllipsoidPlanner, control_lattice, prior_from_traj, state13
from tests import cloud_checker as CC
from tests import cloud_prior_checker as PC

ORI, DIM, R = (-3.37, 2.21, -0.52), (12.0, 6.0, 2.0), 0.5
DT, V_MAX, A_MAX, W = 0.4, 3.0, 20.0, 1000.0
U_OF = {VEL: 2.5, ACC: 5.0, JRK: 10.0, SNP: 20.0}
TOL = (1.0, 2.0, 100.0)
MAX_NUM = 300
LDS_CAP = 256  # CLOUD_PRIOR_LDS_CAP of mplx_cloud.h


def at(*rel):
    return tuple(float(o + x) for o, x in zip(ORI, rel))


def room():
    """a wall in the plane x = 6 with a doorway 2.25 < y < 3.75, points every 0.25 m (relative to the box origin)"""
    ys = [0.25 * i for i in range(25) if not 2.25 < 0.25 * i < 3.75]
    pts = np.array([at(6.0, y, 0.25 * k) for y in ys for k in range(9)])
    assert len(pts) == 180
    return pts


_cache = {}


def checker(control):
    if ("ck", control) not in _cache:
        cloud = CC.Cloud(room(), R, ORI, DIM)
        _cache[("ck", control)] = PC.Checker(cloud, control, control_lattice(U_OF[control], 1, False), DT, v_max=V_MAX, a_max=A_MAX, w=W)
    return _cache[("ck", control)]


def device(control):
    pl = EllipsoidPlanner(False)
    pl.set_map(room(), R, ORI, DIM)
    pl.set_control(control)
    pl.set_u(control_lattice(U_OF[control], 1, False))
    pl.set_dt(DT); pl.set_vmax(V_MAX); pl.set_amax(A_MAX); pl.set_w(W)
    pl.set_tol(*TOL)
    pl.set_max_num(MAX_NUM)
    pl.set_capacity(8, 1 << 18, 1 << 20, 1 << 18)
    pl.set_record(1 << 12)
    return pl


def line_prior(p0, p1, speed, control=ACC, T=None, dt=DT, w=W):
    """P1 of a straight run from p0 towards p1 at `speed` (T: its duration, the time to p1 by default)"""
    p0, p1 = np.array(p0, dtype=np.float64), np.array(p1, dtype=np.float64)
    d = (p1 - p0) / np.linalg.norm(p1 - p0)
    T = float(np.linalg.norm(p1 - p0) / speed) if T is None else T
    return PC.sample_prior(lambda t: list(p0 + d * (speed * t)) + list(d * speed) + [0.0] * 6, T, dt, w, control)


def head(prior, n):
    return {k: v[:n].copy() for k, v in prior.items()}


START, GOAL = at(2.0, 1.0, 1.0), at(10.0, 4.5, 1.0)
DOOR = at(6.0, 3.0, 1.0)
NEAR = (state13(at(4.0, 3.0, 1.0)), state13(at(8.0, 3.0, 1.0)))  # a short query straight through the doorway
KW = dict(tol_pos=TOL[0], tol_vel=TOL[1], tol_acc=TOL[2], max_num=MAX_NUM)


def plan_prior(control, eps=2.0):
    """the hierarchical use: the plan of START -> GOAL in a cheaper control kind, sampled as a prior (P1)"""
    if ("prior", control) not in _cache:
        ck = checker(control)
        c = ck.plan(state13(START), state13(GOAL), eps=eps, **KW)
        assert c["status"] == 0
        _cache[("prior", control)] = prior_from_traj(c["traj"]["states"], c["traj"]["actions"], ck.U, control, DT, W)
    return _cache[("prior", control)]


def extend(prior, n):
    """the table continued to n entries that hold its last state at no cost-to-go"""
    m = n - len(prior["cost_to_go"])
    st = np.repeat(prior["states"][-1:], m, axis=0)
    st[:, 12] = prior["states"][-1, 12] + DT * np.arange(1, m + 1)
    return {"states": np.concatenate([prior["states"], st]), "controls": np.concatenate([prior["controls"], np.repeat(prior["controls"][-1:], m)]),
            "cost_to_go": np.concatenate([prior["cost_to_go"], np.zeros(m)])}


# name -> (control, start13, goal13, prior, eps): the whole-plan cases
PLAN_CASES = {
    # the first half of the ACC plan (5 entries): the heuristic aims at it, then at the goal
    "short": (JRK, state13(START), state13(GOAL), lambda: head(plan_prior(ACC), 5), 2.0),
    # the ACC plan held at its end: 30 entries, more than the plan has steps; guiding a JRK and an ACC search
    "long": (JRK, NEAR[0], NEAR[1], lambda: extend(plan_prior(ACC), 30), 2.0),
    "long_acc": (ACC, state13(START), state13(GOAL), lambda: extend(plan_prior(ACC), 30), 2.0),
    # ... and 400 entries, past the LDS staging cap
    "long_400": (ACC, state13(START), state13(GOAL), lambda: extend(plan_prior(ACC), 400), 2.0),
    # (P4) the start is two steps into the prior
    "start_t": (JRK, state13(START, t=2 * DT), state13(GOAL), lambda: plan_prior(ACC), 2.0),
    "eps0": (VEL, NEAR[0], NEAR[1], lambda: plan_prior(VEL), 0.0),
    "eps1": (JRK, NEAR[0], NEAR[1], lambda: head(plan_prior(ACC), 5), 1.0),
    # eps 1 on the long query: stops at the cap of 300 expansions, with re-opened states on the way
    "eps1_capped": (ACC, state13(START), state13(GOAL), lambda: plan_prior(VEL), 1.0),
    # leads away from the goal, into the corner behind the start: an inconsistent heuristic, states re-open
    "misleading": (ACC, state13(START), state13(GOAL), lambda: line_prior(START, at(0.5, 5.5, 1.0), 2.5, T=4.0), 2.0),
    "snp": (SNP, NEAR[0], NEAR[1], lambda: head(plan_prior(ACC), 5), 2.0),
    "vel": (VEL, state13(START), state13(GOAL), lambda: plan_prior(ACC), 2.0),
}


def reference(name):
    """the checker's plan of a case: computed once, shared, never modified"""
    if ("ref", name) not in _cache:
        control, start, goal, prior, eps = PLAN_CASES[name]
        prior = prior()
        c = checker(control).plan(start, goal, prior=prior, eps=eps, **KW)
        _cache[("ref", name)] = (prior, c)
    return _cache[("ref", name)]


def compare(pl, q, c):
    """query q of the device's last batch against a checker result: expansion order, states with their t, g, flags, trajectory"""
    r = pl.result(q)
    assert r["status"] == c["status"]
    assert r["n_expanded"] == len(c["expanded"])
    assert r["expand_hash"] == CC.expand_hash(c["expanded"])
    assert list(pl.expanded_ids(q)) == c["expanded"]
    assert r["n_nodes"] == len(c["states"])
    st, g, closed, opened = pl.nodes(q)
    assert np.array_equal(st, np.array(c["states"]))
    assert np.array_equal(g, np.array(c["g"]))
    assert closed.tolist() == c["closed"] and opened.tolist() == c["opened"]
    assert r["n_reopen"] == c["n_reopen"]
    if c["status"] == 0:
        assert r["cost"] == c["cost"]
        tr = pl.get_traj(q)
        assert tr["node_ids"].tolist() == c["traj"]["node_ids"]
        assert tr["actions"].tolist() == c["traj"]["actions"]
        assert np.array_equal(tr["states"], c["traj"]["states"])
    return r


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_checker_vel_to_vel_entry_is_the_hand_computed_value():
    """P2 by hand: a VEL state towards a VEL entry costs (w + 1) |dp| + cost_to_go; past the table, (w + 1) |goal - p|"""
    U = control_lattice(1.0, 1, False)
    goal = state13((10.0, 0.0, 0.0))
    prior = {"states": np.array([state13((0.0, 0.0, 0.0)), state13((3.0, 4.0, 0.0), t=0.5)]), "controls": np.array([VEL, VEL], dtype=np.int32),
             "cost_to_go": np.array([7.0, 2.5])}
    h = PC.PriorHeuristic(VEL, U, 0.5, -1.0, 10.0, goal, prior)
    assert h(state13((0.0, 0.0, 0.0), t=0.5)) == 11.0 * 5.0 + 2.5  # entry 1: |(3, 4, 0)| = 5
    assert h(state13((3.0, 0.0, 0.0), t=0.25)) == 11.0 * 3.0 + 7.0  # entry 0
    assert h(state13((0.0, 0.0, 0.0), t=1.0)) == 11.0 * 10.0  # id 2 == n: the goal
    assert h(state13((0.0, 0.0, 0.0), t=-0.5)) == 11.0 * 10.0
    assert h(state13((0.0, 0.0, 0.0), t=math.nan)) == 11.0 * 10.0
    assert h(state13((10.0, 0.0, 0.0), t=0.5)) == 0.0  # the goal's key


def test_checker_with_an_empty_prior_is_the_plain_checker():
    ck = checker(ACC)
    plain = CC.Checker(ck.cloud, ACC, ck.U, DT, v_max=V_MAX, a_max=A_MAX, w=W)
    kw = dict(eps=2.0, **KW)
    a = plain.plan(state13(START), state13(GOAL), **kw)
    for prior in (None, head(line_prior(START, DOOR, 1.2), 0)):
        b = ck.plan(state13(START), state13(GOAL), prior=prior, **kw)
        assert a["status"] == b["status"] == 0 and a["cost"] == b["cost"] and a["expanded"] == b["expanded"]
        assert np.array_equal(np.array(a["states"]), np.array(b["states"])) and a["g"] == b["g"]
        assert a["closed"] == b["closed"] and a["opened"] == b["opened"] and a["n_reopen"] == b["n_reopen"]
        assert a["traj"]["node_ids"] == b["traj"]["node_ids"] and a["traj"]["actions"] == b["traj"]["actions"]


def test_sampling_accumulates_t_by_repeated_addition():
    """P1: t = 0, dt, dt + dt, ...; an entry as long as t < T; cost_to_go w (T - t)"""
    p = PC.sample_prior(lambda t: [t] + [0.0] * 11, 0.8, 0.1, 10.0, ACC)
    ts = [0.0]
    while ts[-1] + 0.1 < 0.8:
        ts.append(ts[-1] + 0.1)
    assert ts[3] == 0.30000000000000004 and ts[-1] == 0.7999999999999999 and len(ts) == 9  # (eight additions stay below 0.8)
    assert p["states"][:, 12].tolist() == ts and p["states"][:, 0].tolist() == ts
    assert p["cost_to_go"].tolist() == [10.0 * (0.8 - t) for t in ts]
    from mpl_ros_amd.ellipsoid import prior_from_traj
    q = prior_from_traj(np.array([state13((1.0, 2.0, 3.0), vel=(0.5, 0.0, 0.0)), state13((0, 0, 0))]), [0], [(2.0, 0.0, 0.0)], ACC, 0.1, 10.0, seg_dt=0.8)
    assert q["states"][:, 12].tolist() == ts and q["controls"].tolist() == [ACC] * 9 and q["cost_to_go"].tolist() == p["cost_to_go"].tolist()
    assert q["states"][3, 0] == 2.0 / 2 * ts[3] * ts[3] + 0.5 * ts[3] + 1.0 and q["states"][3, 3] == 2.0 * ts[3] + 0.5 and q["states"][3, 6] == 2.0


def test_the_misleading_prior_reopens_states_on_the_checker():
    """the inconsistent-heuristic paths are really exercised by the GPU case of the same name"""
    _, c = reference("misleading")
    assert c["status"] == 0 and c["n_reopen"] > 0 and len(c["expanded"]) <= MAX_NUM


def test_the_plan_cases_cover_shorter_and_longer_priors_on_the_checker():
    for name in PLAN_CASES:
        prior, c = reference(name)
        assert 3 < len(c["expanded"]) <= MAX_NUM and c["status"] == (3 if name == "eps1_capped" else 0), name
        if name in ("short", "long", "long_acc", "long_400"):
            steps = len(c["traj"]["actions"])
            assert (len(prior["cost_to_go"]) < steps) == (name == "short"), (name, len(prior["cost_to_go"]), steps)
    assert reference("eps1_capped")[1]["n_reopen"] > 0


def test_python_refuses_a_missing_trajectory_with_the_old_text():
    class Stub(EllipsoidPlanner):
        def __init__(self):
            pass
    with pytest.raises(_capi.MplxError, match="prior trajectories are not supported"):
        Stub().set_prior_trajectory(None)


# ------------------------------------------------------------------------------------------------- GPU: the heuristic entry
def boundary_times(dt, n):
    s3 = dt + dt + dt
    under = 0.0
    for _ in range(n):
        under += dt  # n additions of 0.1 land just under n dt
    return [0.0, -0.0, dt, s3, 3 * dt, under, n * dt, (n - 1) * dt, (n - 0.5) * dt, -dt, -1e-300, 1e300, math.inf, -math.inf, math.nan, 2.5 * dt]


@pytest.mark.gpu
@pytest.mark.parametrize("control", [VEL, ACC, JRK, SNP])
@pytest.mark.parametrize("hid", [False, True])
def test_heuristic_entry_on_index_boundaries_and_control_pairings(control, hid):
    """dt = 0.1, a table of 8 entries whose control kinds cycle VEL, ACC, JRK, SNP: every state time of boundary_times against
    states of the planner's kind, so that each pairing of kinds and each side of each index boundary is evaluated"""
    dt, n = 0.1, 8
    assert 0.1 + 0.1 + 0.1 > 0.3 and boundary_times(dt, n)[5] < 0.8 and int(boundary_times(dt, n)[5] / dt) == n - 1
    rng = np.random.default_rng(7 + control)
    prior = {"states": np.c_[rng.uniform(-4, 4, (n, 3)), rng.uniform(-2, 2, (n, 9)), dt * np.arange(n)],
             "controls": np.array([VEL, ACC, JRK, SNP] * 2, dtype=np.int32), "cost_to_go": rng.uniform(0, 50, n)}
    goal = state13((5.0, -3.0, 1.0), vel=(0.5, 0.0, 0.0), acc=(0.0, 0.25, 0.0))
    pl = device(control)
    pl.set_dt(dt)
    pl.set_heur_ignore_dynamics(hid)
    assert pl.plan(goal, goal) and pl.result()["n_expanded"] == 0  # (the entry uses the flag of the last plan)
    pl.set_prior_trajectory(prior)
    states = []
    for t in boundary_times(dt, n):
        for _ in range(3):
            states.append(state13(rng.uniform(-4, 4, 3), vel=rng.uniform(-2, 2, 3), acc=rng.uniform(-2, 2, 3), jrk=rng.uniform(-2, 2, 3), t=t))
    for t in (0.0, 0.35, 0.8, -1.0):  # the goal's key, inside and outside the table
        g = goal.copy()
        g[12] = t
        g[0] += 0.002  # (the same key: positions are keyed in steps of 0.01)
        states.append(g)
    states = np.array(states)
    ref = PC.PriorHeuristic(control, control_lattice(U_OF[control], 1, False), dt, V_MAX, W, goal * checker(control).mask, prior, heur_ignore_dynamics=hid)
    want = np.array([ref(s * checker(control).mask) for s in states])
    got = pl.heuristic_batch(states, goal)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert (want[-4:] == 0.0).all() and (want[:-4] > 0.0).all()
    # and without a prior: get_heur towards the goal
    pl.clear_prior_trajectory()
    none = PC.PriorHeuristic(control, control_lattice(U_OF[control], 1, False), dt, V_MAX, W, goal * checker(control).mask, None, heur_ignore_dynamics=hid)
    assert np.array_equal(pl.heuristic_batch(states, goal), np.array([none(s * checker(control).mask) for s in states]))
    with pytest.raises(_capi.MplxError):
        pl.heuristic_batch(states, goal, set=1)


# ------------------------------------------------------------------------------------------------------- GPU: whole plans
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLAN_CASES))
def test_guided_plan_equals_the_checker(name):
    control, start, goal, _, eps = PLAN_CASES[name]
    prior, c = reference(name)
    pl = device(control)
    pl.set_epsilon(eps)
    pl.set_prior_trajectory(prior)
    pl.plan(start, goal)
    r = compare(pl, 0, c)
    assert r["n_expanded"] <= MAX_NUM
    if name == "misleading":
        assert r["n_reopen"] > 0
    # the prior changed the search: without it the expansion order differs (eps 0 has no heuristic at all)
    pl.clear_prior_trajectory()
    pl.plan(start, goal)
    assert (pl.result()["expand_hash"] == r["expand_hash"]) == (name == "eps0")


@pytest.mark.gpu
def test_tables_below_and_above_the_lds_cap_give_one_result():
    """the same leading entries staged in LDS (up to the cap) and read from global memory (cap + 1 and 400 entries): no state of
    the search is as late as the cap, so the plan never sees the difference"""
    control, start, goal, _, eps = PLAN_CASES["long_400"]
    prior, c = reference("long_400")
    assert len(prior["cost_to_go"]) == 400 > LDS_CAP and c["status"] == 0 and max(s[12] for s in c["states"]) / DT + 2 < LDS_CAP
    pl = device(control)
    pl.set_epsilon(eps)
    for n in (LDS_CAP - 1, LDS_CAP, LDS_CAP + 1, 400):
        pl.set_prior_trajectory(head(prior, n))
        pl.plan(start, goal)
        compare(pl, 0, c)


# ------------------------------------------------------------------------------------------------- GPU: batches and the API
def batch_queries():
    """8 queries (ACC), each with its own prior; queries 2 and 5 have none"""
    rels = [((2.0, 1.0), (10.0, 4.5)), ((1.5, 5.0), (10.5, 1.0)), ((2.0, 3.0), (9.0, 3.0)), ((10.0, 1.0), (2.0, 5.0)),
            ((3.0, 0.8), (9.5, 5.2)), ((10.5, 5.0), (1.5, 0.8)), ((4.0, 4.5), (8.0, 1.5)), ((1.0, 1.0), (11.0, 5.0))]
    starts = [state13(at(a[0], a[1], 1.0)) for a, _ in rels]
    goals = [state13(at(b[0], b[1], 1.0)) for _, b in rels]
    priors = [None if q in (2, 5) else line_prior(s[:3], DOOR, 1.0 + 0.2 * q, control=(VEL, ACC)[q % 2]) for q, s in enumerate(starts)]
    return starts, goals, priors


KEYS = ("status", "cost", "n_expanded", "n_closed", "n_nodes", "n_edges", "n_succ", "n_push", "n_reopen", "expand_hash", "traj_len")


def snapshot(pl, q):
    r = pl.result(q)
    tr = pl.get_traj(q)
    return ({k: r[k] for k in KEYS}, [a.tobytes() for a in pl.nodes(q)], None if tr is None else [tr[k].tobytes() for k in ("states", "actions", "node_ids")])


@pytest.mark.gpu
def test_batch_of_eight_priors_equals_the_eight_alone_and_the_checker():
    starts, goals, priors = batch_queries()
    pl = device(ACC)
    pl.set_epsilon(2.0)
    pl.plan_batch(starts, goals, priors=priors)
    together = [snapshot(pl, q) for q in range(8)]
    ck = checker(ACC)
    for q in (0, 2, 7):  # (the checker is slow: three of them, one without a prior)
        compare(pl, q, ck.plan(starts[q], goals[q], prior=priors[q], eps=2.0, **KW))
    one = device(ACC)
    one.set_epsilon(2.0)
    for q in range(8):
        one.plan_batch(starts[q:q + 1], goals[q:q + 1], priors=priors[q:q + 1])
        assert snapshot(one, 0) == together[q], q
    assert len({t[0]["expand_hash"] for t in together}) == 8


@pytest.mark.gpu
def test_set_count_must_match_the_batch_and_nothing_is_launched():
    starts, goals, priors = batch_queries()
    pl = device(ACC)
    pl.set_epsilon(2.0)
    pl.plan_batch(starts[:2], goals[:2])
    before = [snapshot(pl, q) for q in range(2)]
    pl.set_priors(priors[:3])
    out = (_capi.Result * 2)()
    s, g = np.ascontiguousarray(starts[:2]), np.ascontiguousarray(goals[:2])
    code = pl.lib.mplx_cloud_plan_batch(pl.h, 2, s.ctypes.data, g.ctypes.data, 2.0, TOL[0], TOL[1], TOL[2], MAX_NUM, 0, out)
    assert code == _capi.ERR_ARG and b"prior sets" in pl.lib.mplx_cloud_last_error(pl.h)
    assert [snapshot(pl, q) for q in range(2)] == before  # (the last batch's results still stand: nothing ran)
    with pytest.raises(_capi.MplxError):
        pl.plan_batch(starts[:2], goals[:2])
    pl.plan_batch(starts[:3], goals[:3])  # three sets, three queries
    assert pl.result(2)["status"] in (_capi.PLAN_OK, _capi.PLAN_MAX_EXPAND)


@pytest.mark.gpu
def test_prior_persists_until_cleared_and_clearing_restores_the_plain_search():
    control, start, goal, _, eps = PLAN_CASES["short"]
    prior, c = reference("short")
    pl = device(control)
    pl.set_epsilon(eps)
    pl.plan(start, goal)
    plain = snapshot(pl, 0)
    pl.set_prior_trajectory(prior)
    pl.plan(start, goal)
    first = snapshot(pl, 0)
    pl.plan(start, goal)
    assert snapshot(pl, 0) == first and first != plain
    compare(pl, 0, c)
    pl.clear_prior_trajectory()
    pl.plan(start, goal)
    assert snapshot(pl, 0) == plain


@pytest.mark.gpu
def test_values_that_are_not_finite_are_refused():
    prior = line_prior(START, DOOR, 1.2)
    assert len(prior["cost_to_go"]) >= 10
    pl = device(ACC)
    for key, idx in (("states", (3, 4)), ("cost_to_go", 5)):
        for bad in (math.nan, math.inf):
            p = head(prior, 10)
            p[key][idx] = bad
            with pytest.raises(_capi.MplxError, match="not finite"):
                pl.set_prior_trajectory(p)
    p = head(prior, 10)
    p["controls"][2] = 5
    with pytest.raises(_capi.MplxError, match="control kind"):
        pl.set_prior_trajectory(p)
