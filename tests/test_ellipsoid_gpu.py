"""GPU: the point-cloud planner (mplx_cloud_*, mpl_ros_amd/ellipsoid.py) bit for bit against the CPU checker
(tests/cloud_checker.py): env_cloud::get_succ on several clouds, the office-shaped plan with the launch file's parameters,
the expansion cap, a batch of 64 queries, and a pool too small for the search."""
import math
import time

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd.ellipsoid import EllipsoidPlanner, control_lattice, state13
from oracle import orc
from tests import cloud_checker as K
from tests import cloud_scenes as S
from tests.cloud_compare import _compare_plan, _compare_succ

pytestmark = pytest.mark.gpu

L = S.LAUNCH
BOX = ((0.0, 0.0, 0.0), (10.0, 10.0, 3.0))


def _planner(pts, r, ori, dim, control, U, **kw):
    pl = EllipsoidPlanner(False)
    pl.set_map(pts, r, ori, dim)
    pl.set_control(control)
    pl.set_u(U)
    pl.set_dt(kw.get("dt", 0.2)); pl.set_vmax(kw.get("v_max", 10.0)); pl.set_amax(kw.get("a_max", 10.0))
    pl.set_jmax(kw.get("j_max", -1.0)); pl.set_w(kw.get("w", 10.0))
    ck = K.Checker(K.Cloud(pts, r, ori, dim), control, U, kw.get("dt", 0.2), v_max=kw.get("v_max", 10.0), a_max=kw.get("a_max", 10.0),
                   j_max=kw.get("j_max", -1.0), w=kw.get("w", 10.0))
    return pl, ck


def _random_states(rng, n, lo, hi, control, vmax=6.0, amax=6.0):
    st = np.zeros((n, 13))
    st[:, 0:3] = rng.uniform(lo, hi, size=(n, 3))
    st[:, 3:6] = rng.uniform(-vmax, vmax, size=(n, 3))
    if control & 4:
        st[:, 6:9] = rng.uniform(-amax, amax, size=(n, 3))
    st[:, 12] = rng.uniform(0, 5, size=n)
    return st


def _sampled_ellipsoid(ck, s13, i, j, r):
    """ellipsoid j of the n + 1 that isFree tests on primitive (s13, U[i]): centre, C, b3, n (E6)"""
    w = K.state_wp(s13, ck.control)
    pr = orc.Primitive()
    orc.lib().orc_primitive_build(K.C.byref(w), (K.C.c_double * 3)(*ck.U[i]), ck.dt, K.C.byref(pr))
    mv = max([0.0] + [orc.lib().orc_primitive_max_vel(K.C.byref(pr), k) for k in range(3)])
    n = int(math.ceil(mv * ck.dt / r))
    j = min(j, n)
    e = orc.Waypoint()
    orc.lib().orc_primitive_evaluate(K.C.byref(pr), 0.0 if n == 0 else j * (ck.dt / n), K.C.byref(e))
    Cm, (b1, b2, b3) = K.ellipsoid_C((r, r, 0.1), list(e.acc))
    return np.array(e.pos), np.array(Cm), np.array(b3), n


def _near_surface_cloud(rng, ck, states, r, n_pts=400):
    """points just inside and just outside ellipsoids that isFree tests (sample t = j (dt / n) of a primitive of `states`):
    ||C^-1 (p - d)|| = 1 -+ 1e-6 and 1 -+ 1e-3"""
    pts = []
    for s13 in states[: n_pts // 4]:
        i = int(rng.integers(len(ck.U)))
        d, Cm, _, n = _sampled_ellipsoid(ck, s13, i, int(rng.integers(0, 64)), r)
        for sgn in (1 - 1e-6, 1 + 1e-6, 1 - 1e-3, 1 + 1e-3):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            pts.append(d + Cm @ (u * sgn))
    return np.array(pts)


@pytest.mark.parametrize("control", [orc.ACC, orc.JRK])
@pytest.mark.parametrize("use_3d", [False, True])
def test_get_succ_office(control, use_3d):
    rng = np.random.default_rng(10 + control + 100 * use_3d)
    U = control_lattice(60.0 if control == orc.ACC else 200.0, 2 if not use_3d else 1, use_3d, 20.0)
    pts = S.office()
    pl, ck = _planner(pts, 0.5, S.ORI, S.DIM, control, U, a_max=40.0 if control == orc.JRK else 10.0)
    states = _random_states(rng, 150, (6.5, 12.5, 0.8), (30.5, 16.5, 1.4), control)
    n_valid = _compare_succ(pl, ck, states)
    assert 0 < n_valid < states.shape[0] * len(U)


@pytest.mark.parametrize("control", [orc.ACC, orc.JRK])
def test_get_succ_near_surface_points(control):
    rng = np.random.default_rng(3 + control)
    U = control_lattice(30.0, 1, True, 10.0)
    states = _random_states(rng, 200, (2, 2, 1), (8, 8, 2), control, vmax=3.0, amax=3.0)
    ck0 = K.Checker(K.Cloud([], 0.5, *BOX), control, U, 0.2, v_max=10.0, a_max=20.0)
    pts = _near_surface_cloud(rng, ck0, states, 0.5)
    pl, ck = _planner(pts, 0.5, BOX[0], BOX[1], control, U, a_max=20.0)
    n_valid = _compare_succ(pl, ck, states)
    assert 0 < n_valid < states.shape[0] * len(U)


def test_get_succ_flat_robot_outside_point_empty_and_outlier():
    rng = np.random.default_rng(7)
    U = control_lattice(20.0, 1, False)
    states = _random_states(rng, 200, (0.3, 0.3, 0.3), (9.7, 9.7, 2.7), orc.ACC, vmax=2.0)
    ck0 = K.Checker(K.Cloud([], 0.05, *BOX), orc.ACC, U, 0.2, v_max=10.0)
    pts = _near_surface_cloud(rng, ck0, states, 0.05)  # r = 0.05 < h: the radius filter truncates the ellipsoid
    pl, ck = _planner(pts, 0.05, BOX[0], BOX[1], orc.ACC, U)
    _compare_succ(pl, ck, states)
    # a far outlier next to every other case, and an empty cloud
    pl, ck = _planner(np.concatenate([pts, [[1e4, -1e4, 5e3]]]), 0.05, BOX[0], BOX[1], orc.ACC, U)
    _compare_succ(pl, ck, states[:60])
    pl, ck = _planner(np.zeros((0, 3)), 0.5, BOX[0], BOX[1], orc.ACC, U)
    assert _compare_succ(pl, ck, states[:60]) > 0


def test_get_succ_truncated_pole_point_does_not_block():
    """r = 0.05 < h = 0.1: a point 0.9 h from a tested sample centre along b3 is inside that ellipsoid but outside the search
    radius (and farther than r from every other sample centre, all at its height), so the primitive stays free; at 0.04 it
    blocks"""
    U = control_lattice(20.0, 1, False)
    s = state13((5.0, 5.0, 1.5), vel=(1.0, 0.0, 0.0))
    i = [tuple(u) for u in U.tolist()].index((0.0, 0.0, 0.0))  # (coasting along x: b3 vertical, every centre at z = 1.5)
    ck0 = K.Checker(K.Cloud([], 0.05, *BOX), orc.ACC, U, 0.2, v_max=10.0)
    d, Cm, b3, n = _sampled_ellipsoid(ck0, s, i, 2, 0.05)
    assert n >= 2
    pole = d + 0.09 * b3
    assert K.inside(K.inverse3(Cm.tolist()), d.tolist(), pole[None, :])[0]
    assert np.dot(pole - d, pole - d) > 0.05 ** 2
    for p, free in ((pole, True), (d + 0.04 * b3, False)):
        pl, ck = _planner(p[None, :], 0.05, BOX[0], BOX[1], orc.ACC, U)
        valid, _, _, _ = pl.get_succ_batch(s[None, :])
        assert bool(valid[0, i]) == free
        _compare_succ(pl, ck, s[None, :])


def test_get_succ_point_outside_the_box_blocks():
    """every point is kept (setObstacles before setBoundingBox): a point at x = -0.02, outside the box, blocks the primitive
    that ends at x = 0.05 and is free without it"""
    U = control_lattice(20.0, 1, False)
    st = np.array([state13((0.45, 5.0, 1.0))])
    i = [tuple(u) for u in U.tolist()].index((-20.0, 0.0, 0.0))
    pl, ck = _planner(np.zeros((0, 3)), 0.5, BOX[0], BOX[1], orc.ACC, U)
    valid, succ, _, _ = pl.get_succ_batch(st)
    assert valid[0, i] == 1 and abs(succ[0, i, 0] - 0.05) < 1e-12
    for cloud in (np.array([[-0.02, 5.0, 1.0]]), np.array([[-0.02, 5.0, 1.0], [1e4, -1e4, 5e3]])):
        pl, ck = _planner(cloud, 0.5, BOX[0], BOX[1], orc.ACC, U)
        valid, _, _, _ = pl.get_succ_batch(st)
        assert valid[0, i] == 0
        _compare_succ(pl, ck, st)


def _office_planner(control=orc.ACC, use_3d=False):
    U = control_lattice(L["u_max"], L["num"], use_3d, 1.0)
    pl, ck = _planner(S.office(), L["r"], S.ORI, S.DIM, control, U, dt=L["dt"], v_max=L["v_max"], a_max=L["a_max"], w=L["w"])
    pl.set_capacity(1, 1 << 21, 1 << 23, 1 << 22)
    pl.set_epsilon(L["eps"])
    pl.set_tol(*L["tol"])
    return pl, ck


def test_office_plan_matches_the_checker():
    pl, ck = _office_planner()
    t0 = time.time()
    r, c = _compare_plan(pl, ck, state13(S.START), state13(S.GOAL))
    assert r["status"] == _capi.PLAN_OK
    print(f"office: cost {r['cost']} expanded {r['n_expanded']} point tests {r['voxel_reads']} kernel {pl.last_kernel_ms():.3f} ms")


def test_office_plan_max_num():
    pl, ck = _office_planner()
    r, c = _compare_plan(pl, ck, state13(S.START), state13(S.GOAL), max_num=12)
    assert r["status"] == _capi.PLAN_MAX_EXPAND and r["n_expanded"] == 12


@pytest.mark.parametrize("control,use_3d,max_num", [(orc.JRK, False, 3000), (orc.ACC, True, 400)])
def test_office_plan_jrk_and_3d_lattice_match_the_checker(control, use_3d, max_num):
    """JRK states (the node's default start: use_acc) and a use_3d lattice; both re-open closed states (D6, eps = 2)"""
    pl, ck = _office_planner(control, use_3d)
    r, c = _compare_plan(pl, ck, state13(S.START), state13(S.GOAL), max_num=max_num)
    assert c["n_reopen"] > 0 and r["n_reopen"] > 0


def _free_pairs(rng, n):
    xs = [7.5, 10.0, 14.0, 16.0, 20.0, 22.0, 26.0, 29.5]
    starts, goals = [], []
    for _ in range(n):
        a, b = rng.choice(len(xs), 2, replace=False)
        starts.append(state13((xs[a], rng.uniform(13.0, 16.0), 1.3)))
        goals.append(state13((xs[b], rng.uniform(13.0, 16.0), 1.3)))
    return np.array(starts), np.array(goals)


def test_batch_of_64_equals_single_queries_and_the_checker():
    rng = np.random.default_rng(64)
    starts, goals = _free_pairs(rng, 64)
    pl, ck = _office_planner()
    pl.set_max_num(3000)
    pl.set_capacity(64, 1 << 23, 1 << 25, 1 << 23)  # (room for every query of the batch at its cap)
    batch = pl.plan_batch(starts, goals)
    trajs = [pl.get_traj(q) for q in range(64)]
    assert sum(b["status"] == _capi.PLAN_OK for b in batch) >= 32
    for q in range(64):
        one = pl.plan_batch(starts[q:q + 1], goals[q:q + 1])[0]
        for k in ("status", "cost", "n_expanded", "n_nodes", "expand_hash", "traj_len"):
            assert one[k] == batch[q][k], (q, k)
        t1 = pl.get_traj()
        assert (t1 is None) == (trajs[q] is None)
        if t1 is not None:
            assert np.array_equal(t1["states"], trajs[q]["states"])
    for q in range(0, 64, 8):
        c = ck.plan(starts[q], goals[q], eps=L["eps"], tol_pos=L["tol"][0], tol_vel=L["tol"][1], tol_acc=L["tol"][2], max_num=3000)
        assert batch[q]["status"] == c["status"] and batch[q]["n_expanded"] == len(c["expanded"])
        assert batch[q]["expand_hash"] == K.expand_hash(c["expanded"])
        if c["status"] == 0:
            assert batch[q]["cost"] == c["cost"]
            assert np.array_equal(trajs[q]["states"], c["traj"]["states"])


def test_small_pool_reports_pool_full_within_the_deadline():
    pl, _ = _office_planner()
    pl.set_u(control_lattice(10.0, 5, False))  # a fine lattice: velocities in steps of 0.4, far more states than one chunk holds
    pl.set_epsilon(0.0)  # uniform-cost search towards an unreachable goal
    pl.set_tol(0.01, 0.01, 100.0)
    pl.set_capacity(1, 1 << 15, 1 << 16, 1 << 15)
    pl.set_deadline(60.0)
    t0 = time.time()
    pl.plan(state13(S.START), state13((28.5, 14.0, 1.3), vel=(9.9, 9.9, 0.0)))
    assert pl.result()["status"] == _capi.PLAN_POOL_FULL
    assert time.time() - t0 < 60.0
