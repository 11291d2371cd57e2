"""3-D moving-obstacle planner (PolyMapPlanner3D): mplx_poly3_* against the CPU checker tests/cpp/poly_checker.cpp.

The checker restates env_poly_map / PolyMapUtil / collide() / the obstacle classes templated on Dim.  CPU: at Dim = 2 it agrees
bit for bit with oracle/_ref/libpolymap_ref.so (the reference's own headers compiled) on get_succ and on whole plans, and at
Dim = 3 with oracle/_ref/libpolymap3_ref.so (the same headers instantiated at three dimensions) on the worlds of this file; the
named 3-D scenes are in tests/test_poly3_geometry.py.  -m gpu: the HIP kernels against the checker at Dim = 3, bit-exact (the
comparison bodies are those of tests/poly_compare.py)."""
import ctypes as C

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd import poly_map as pm
from mpl_ros_amd import poly_map3d as p3
from oracle import refpoly
from tests import poly_checker as pc
from tests.poly_compare import compare_get_succ, compare_plans, same_plan as _same_plan, same_succ as _same_succ
from tests.test_poly_map import random_states, random_states_general, random_world, random_world_general

needs_ref = pytest.mark.skipif(not refpoly.available(), reason="oracle/_ref/libpolymap_ref.so (Dim = 2; Dim = 3 is libpolymap3_ref.so) not built (make -C oracle ref)")
needs_ref3 = pytest.mark.skipif(not refpoly.available(3), reason="oracle/_ref/libpolymap3_ref.so (Dim = 3; Dim = 2 is libpolymap_ref.so) not built (make -C oracle ref)")

U9 = pm.U9


# ---------------------------------------------------------------- CPU
def test_new_symbols_are_exported():
    lib = _capi.load()
    names = [n for n in _capi.EXPORTS if n.startswith("mplx_poly3_")]
    assert len(names) == 19 and "mplx_poly3_result_nodes" in names
    for n in names:
        assert getattr(lib, n) is not None
    assert C.sizeof(_capi.Poly3Succ) == 13 * 8 + 8 + 8


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_capi.MplxError):
        p3.PolyTeam3D()


@needs_ref
@pytest.mark.parametrize("control", [pm.ACC, pm.JRK])
def test_checker_at_dim2_equals_the_compiled_reference_get_succ(control):
    rng = np.random.default_rng(40 + control)
    dt = 0.5
    kw = dict(dt=dt, v_max=2.0, a_max=1.0, j_max=1.5, w=10.0)
    worlds = [random_world_general(rng, dt=dt) for _ in range(3)] + [random_world(rng, dt=dt)] + pm.team2_tick(dt=dt)[0][:2] + \
        [pm.replanner_world(1.5), pm.replanner_world(2.5, turn=True)]
    n_inf = n_fin = 0
    for W in worlds:
        ref, chk = refpoly.RefWorld(W, control, U9, **kw), pc.CheckerWorld(W, control, U9, **kw)
        states = random_states_general(rng, 60, control, dt)
        if W.ori[1] == 0.0:  # (the replanner map spans [0, 20]^2)
            states[:, 0:2] += 5.0
        for s in states:
            a, b = ref.get_succ(s), chk.get_succ(s)
            i, f = _same_succ(b, a)
            n_inf += i; n_fin += f
    assert n_inf > 100 and n_fin > 500


@needs_ref
@pytest.mark.parametrize("control,heur_ignore_dynamics", [(pm.ACC, True), (pm.ACC, False), (pm.JRK, True), (pm.JRK, False)])
def test_checker_at_dim2_equals_the_compiled_reference_plans(control, heur_ignore_dynamics):
    rng = np.random.default_rng(60 + control + int(heur_ignore_dynamics))
    dt = 0.5
    kw = dict(dt=dt, v_max=2.0, a_max=1.0, w=10.0)
    cols = [0, 1, 2, 3, 4, 5, 8] if control == pm.JRK else [0, 1, 2, 3, 8]
    worlds, starts, goals = pm.team2_tick(dt=dt)
    cases = [(worlds[k], starts[k], goals[k]) for k in (0, 5)]
    for _ in range(3):
        W = random_world(rng, dt=dt)
        s, g = np.zeros(9), np.zeros(9)
        s[0:2] = np.round(rng.uniform((0.5, -4.5), (3.0, 4.5)), 1)
        g[0:2] = np.round(rng.uniform((7.0, -4.5), (9.5, 4.5)), 1)
        cases.append((W, s, g))
    s, g = pm.replanner_endpoints()
    cases.append((pm.replanner_world(1.0), s, g))
    n_ok = 0
    for W, s, g in cases:
        ref, chk = refpoly.RefWorld(W, control, U9, **kw), pc.CheckerWorld(W, control, U9, **kw)
        pk = dict(eps=1.0, tol_pos=0.5, max_expand=600 if control == pm.JRK else 2000, heur_ignore_dynamics=heur_ignore_dynamics)
        a, b = ref.plan(s, g, **pk), chk.plan(s, g, **pk)
        _same_plan(a, b, ref, chk, cols)
        n_ok += int(a["status"] == 0)
    assert n_ok >= (2 if control == pm.ACC else 0)


# ---------------------------------------------------------------- 3-D scenes
S3 = 0.5773502691896258  # 1 / sqrt(3)


def octahedron(r):
    """A tilted polyhedron: the eight faces of |x| + |y| + |z| <= r, normals (+-1, +-1, +-1) / sqrt(3)"""
    rows = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                rows.append([sx * r, 0.0, 0.0, sx * S3, sy * S3, sz * S3])
    return np.array(rows)


def random_world3d(rng, jrk_obstacles=False, dt=0.5):
    W = p3.PolyWorld3D((0.0, -5.0, 0.0), (10.0, 10.0, 4.0), start_t=float(rng.choice([0.0, 0.5, 1.25])))
    W.static.append(p3.StaticObstacle3D(p3.box(0.6, 0.8, 1.0), rng.uniform((2, -3, 1), (8, 3, 3))))
    W.static.append(p3.StaticObstacle3D(octahedron(1.0), rng.uniform((2, -3, 1), (8, 3, 3))))
    W.linear.append(p3.LinearObstacle3D(p3.box(0.5), rng.uniform((1, -4, 1), (9, 4, 3)), rng.uniform(-1, 1, 3), cov_v=0.0))
    W.linear.append(p3.LinearObstacle3D(octahedron(0.7), rng.uniform((1, -4, 1), (9, 4, 3)), rng.uniform(-1, 1, 3), cov_v=0.1))
    U27 = p3.control_lattice(1.0, 1)
    for k in range(4):
        n = int(rng.integers(1, 6))
        us = U27[rng.integers(0, len(U27), n)]
        p0, v0 = rng.uniform((1, -4, 1), (9, 4, 3)), np.round(rng.uniform(-1, 1, 3), 1)
        segs = p3.jrk_segs(p0, v0, np.round(rng.uniform(-0.5, 0.5, 3), 1), us, dt) if (jrk_obstacles and k % 2) else p3.acc_segs(p0, v0, us, dt)
        W.nonlinear.append(p3.NonlinearObstacle3D(p3.box(0.5), segs, start_t=float(rng.choice([-0.5, 0.0, 0.3, 2.0, 10.0])),
                                                  disappear_front=bool(rng.integers(0, 2)), disappear_back=bool(rng.integers(0, 2))))
    return W


def random_states3d(rng, W, n, control, dt=0.5):
    s = np.zeros((n, 13))
    s[:, 0:3] = np.round(rng.uniform((0.2, -4.8, 0.2), (9.8, 4.8, 3.8), (n, 3)), 2)
    s[:, 3:6] = np.round(rng.uniform(-1.5, 1.5, (n, 3)), 1)
    if control & 4:
        s[:, 6:9] = np.round(rng.uniform(-0.8, 0.8, (n, 3)), 1)
    s[:, 12] = rng.integers(0, 8, n) * dt
    m = n // 8
    s[0:m, 0] = 0.0                      # on the -x face
    s[m:2 * m, 2] = 4.0                  # on the +z face
    s[2 * m:3 * m, 2] = -0.3             # below the box
    s[3 * m:4 * m, 0:3] = W.static[0].p  # inside a static obstacle
    s[4 * m:5 * m, 0:3] = np.round(s[4 * m:5 * m, 0:3])  # lattice points
    return s


KW3 = dict(dt=0.5, v_max=2.0, a_max=1.5, j_max=2.0, w=10.0)


def _u27():
    return p3.control_lattice(1.0, 1)


SUCC_SETUPS = [(pm.ACC, False), (pm.ACC, True), (pm.JRK, True), (pm.VEL, False)]  # (control, cubic obstacle trajectories) of the GPU test below


def succ_case(control, jrk_obstacles):
    """the worlds and states test_get_succ_batch_equals_the_checker runs on"""
    rng = np.random.default_rng(1000 + 10 * control + int(jrk_obstacles))
    worlds = [random_world3d(rng, jrk_obstacles) for _ in range(4)]
    K = 160
    world_of = np.repeat(np.arange(len(worlds)), K // len(worlds))
    states = np.concatenate([random_states3d(rng, W, K // len(worlds), control) for W in worlds])  # (faces, outside, inside an obstacle)
    return worlds, world_of, states


@needs_ref3
@pytest.mark.parametrize("control,jrk_obstacles", SUCC_SETUPS + [(pm.SNP, True)])
def test_checker_at_dim3_equals_the_compiled_reference_get_succ(control, jrk_obstacles):
    """the very worlds and states of the GPU comparison below (one of them again off the origin), and SNP on top"""
    worlds, world_of, states = succ_case(control, jrk_obstacles)
    far = p3.PolyWorld3D(worlds[0].ori + (-103.7, 41.3, 12.5), worlds[0].dim, worlds[0].start_t)
    shift = np.array([-103.7, 41.3, 12.5])
    far.static = [p3.StaticObstacle3D(o.poly, o.p + shift) for o in worlds[0].static]
    far.linear = [p3.LinearObstacle3D(o.poly, o.p + shift, o.v, o.cov_v) for o in worlds[0].linear]
    for o in worlds[0].nonlinear:
        sg = o.segs.copy()
        sg[:, [5, 11, 17]] += shift
        far.nonlinear.append(p3.NonlinearObstacle3D(o.poly, sg, o.start_t, o.disappear_front, o.disappear_back))
    moved = states[world_of == 0].copy()
    moved[:, 0:3] += shift
    if control == pm.SNP:
        states[:, 9:12] = np.round(np.random.default_rng(7).uniform(-1, 1, (len(states), 3)), 1)
    n_inf = n_fin = 0
    for W, ss in [(W, states[world_of == k]) for k, W in enumerate(worlds)] + [(far, moved)]:
        ref, chk = refpoly.RefWorld3D(W, control, _u27(), **KW3), pc.CheckerWorld(W, control, _u27(), **KW3)
        for s in ss:
            i, f = _same_succ(chk.get_succ(s), ref.get_succ(s))
            n_inf += i; n_fin += f
    assert n_fin > 300 and n_inf > 100


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("control,jrk_obstacles", SUCC_SETUPS)
def test_get_succ_batch_equals_the_checker(control, jrk_obstacles):
    U = _u27()
    worlds, world_of, states = succ_case(control, jrk_obstacles)
    team = p3.PolyTeam3D()
    team.configure(control, U, **KW3)
    team.set_worlds(worlds)
    chks = [pc.CheckerWorld(W, control, U, **KW3) for W in worlds]
    n_fin, n_inf = compare_get_succ(team, worlds, chks, world_of, states, len(U), signs=True)
    assert n_fin > 300 and n_inf > 100


def _plan_cases(rng, n, control, cubic_obstacles=True):
    worlds = [random_world3d(rng, jrk_obstacles=cubic_obstacles and bool(i % 2)) for i in range(4)]
    world_of = rng.integers(0, len(worlds), n)
    starts, goals = np.zeros((n, 13)), np.zeros((n, 13))
    starts[:, 0:3] = np.round(rng.uniform((0.5, -4.5, 0.5), (2.5, 4.5, 3.5), (n, 3)), 1)
    starts[:, 12] = rng.integers(0, 3, n) * 0.5
    goals[:, 0:3] = starts[:, 0:3] + np.round(rng.uniform((1.5, -1.5, -0.5), (3.0, 1.5, 0.5), (n, 3)), 1)
    return worlds, world_of, starts, goals


def _compare_plans(team, chks, world_of, starts, goals, control, **kw):
    return compare_plans(team, chks, world_of, starts, goals, compare_acc=control == pm.JRK, dim=3, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("control,heur_ignore_dynamics", [(pm.ACC, True), (pm.ACC, False), (pm.JRK, True), (pm.JRK, False)])
def test_plans_equal_the_checker(control, heur_ignore_dynamics):
    rng = np.random.default_rng(2000 + control + int(heur_ignore_dynamics))
    U = _u27()
    worlds, world_of, starts, goals = _plan_cases(rng, 8, control)
    team = p3.PolyTeam3D()
    team.configure(control, U, **KW3)
    team.set_worlds(worlds)
    team.set_capacity(8, 1 << 20, 1 << 22, 1 << 21)
    chks = [pc.CheckerWorld(W, control, U, **KW3) for W in worlds]
    R, n_ok = _compare_plans(team, chks, world_of, starts, goals, control, max_expand=1500, heur_ignore_dynamics=heur_ignore_dynamics)
    assert n_ok >= (0 if (control == pm.JRK and heur_ignore_dynamics) else 2)  # (JRK with the distance heuristic: capped searches, compared all the same)


@pytest.mark.gpu
@pytest.mark.parametrize("tol_vel", [-1.0, 0.3])
def test_plans_among_acc_obstacles_equal_the_checker(tol_vel):
    """ACC primitives among static, linear and ACC-trajectory obstacles only: the quadratic build (GEN = false) of the search;
    with tol_vel >= 0 the goal test also bounds the velocity"""
    rng = np.random.default_rng(2500 + int(tol_vel > 0))
    U = _u27()
    worlds, world_of, starts, goals = _plan_cases(rng, 8, pm.ACC, cubic_obstacles=False)
    goals[: len(goals) // 2, 3:6] = np.round(rng.uniform(-1, 1, (len(goals) // 2, 3)), 1)  # (half of the goals carry a velocity)
    team = p3.PolyTeam3D()
    team.configure(pm.ACC, U, **KW3)
    team.set_worlds(worlds)
    team.set_capacity(8, 1 << 20, 1 << 22, 1 << 21)
    chks = [pc.CheckerWorld(W, pm.ACC, U, **KW3) for W in worlds]
    R, n_ok = _compare_plans(team, chks, world_of, starts, goals, pm.ACC, max_expand=1500, heur_ignore_dynamics=False, tol_vel=tol_vel)
    assert n_ok >= (2 if tol_vel < 0 else 1)


@pytest.mark.gpu
def test_cap_pool_full_and_refused_starts():
    rng = np.random.default_rng(3000)
    U = _u27()
    worlds, world_of, starts, goals = _plan_cases(rng, 4, pm.ACC)
    team = p3.PolyTeam3D()
    team.configure(pm.ACC, U, **KW3)
    team.set_worlds(worlds)
    chks = [pc.CheckerWorld(W, pm.ACC, U, **KW3) for W in worlds]
    # the max_num cap
    team.set_capacity(4, 1 << 20, 1 << 22, 1 << 21)
    R, _ = _compare_plans(team, chks, world_of, starts, goals, pm.ACC, max_expand=7)
    assert all(r.status == _capi.PLAN_MAX_EXPAND for r in R)
    # a start outside the bounding box, and one inside an obstacle (PlannerBase only tests the box: it plans, blocked everywhere)
    s2 = starts.copy()
    s2[0, 2] = -0.5
    s2[1, 0:3] = worlds[world_of[1]].static[0].p
    R, _ = _compare_plans(team, chks, world_of, s2, goals, pm.ACC, max_expand=3000)
    assert R[0].status == _capi.PLAN_START_OCCUPIED
    assert R[1].n_expanded == 1 and R[1].status == _capi.PLAN_NO_PATH
    # pools too small: POOL_FULL, reported, never a partial answer
    team.set_capacity(1, 1 << 15, 1 << 17, 1 << 16)
    far = goals.copy()
    far[:, 0:3] = (9.5, 4.5, 3.5)
    R = team.plan_batch(world_of[:1], starts[:1], far[:1], eps=0.0, max_expand=-1)
    assert R[0].status == _capi.PLAN_POOL_FULL and np.isinf(R[0].cost)


@pytest.mark.gpu
def test_batch_of_64_over_16_worlds_equals_one_at_a_time_and_the_checker():
    rng = np.random.default_rng(4000)
    U = _u27()
    worlds = [random_world3d(rng, jrk_obstacles=bool(i % 3 == 0)) for i in range(16)]
    n = 64
    world_of = np.arange(n) % 16
    starts, goals = np.zeros((n, 13)), np.zeros((n, 13))
    starts[:, 0:3] = np.round(rng.uniform((0.5, -4.5, 0.5), (2.5, 4.5, 3.5), (n, 3)), 1)
    goals[:, 0:3] = starts[:, 0:3] + np.round(rng.uniform((1.5, -1.5, -0.5), (3.0, 1.5, 0.5), (n, 3)), 1)
    team = p3.PolyTeam3D()
    team.configure(pm.ACC, U, **KW3)
    team.set_worlds(worlds)
    team.set_capacity(64, 1 << 21, 1 << 23, 1 << 22)
    kw = dict(max_expand=1500)
    team.set_record(1 << 12)
    R = team.plan_batch(world_of, starts, goals, **kw)
    batch = [(r.status, r.cost, r.n_expanded, r.n_nodes, tuple(team.expanded_ids(k)), tuple(team.traj(k)[0])) for k, r in enumerate(R)]
    for k in range(0, n, 5):
        r1 = team.plan_batch(world_of[k:k + 1], starts[k:k + 1], goals[k:k + 1], **kw)[0]
        assert (r1.status, r1.cost, r1.n_expanded, r1.n_nodes, tuple(team.expanded_ids(0)), tuple(team.traj(0)[0])) == batch[k], k
    chks = [pc.CheckerWorld(W, pm.ACC, U, **KW3) for W in worlds]
    R, n_ok = _compare_plans(team, chks, world_of, starts, goals, pm.ACC, **kw)
    assert n_ok >= 8


@pytest.mark.gpu
def test_result_nodes_match_the_checker_state_space():
    rng = np.random.default_rng(5000)
    U = _u27()
    worlds, world_of, starts, goals = _plan_cases(rng, 4, pm.ACC)
    team = p3.PolyTeam3D()
    team.configure(pm.ACC, U, **KW3)
    team.set_worlds(worlds)
    team.set_capacity(4, 1 << 20, 1 << 22, 1 << 21)
    R = team.plan_batch(world_of, starts, goals, max_expand=400)
    for k, w in enumerate(world_of):
        chk = pc.CheckerWorld(worlds[w], pm.ACC, U, **KW3)
        ref = chk.plan(starts[k], goals[k], max_expand=400)
        assert R[k].status == ref["status"] and R[k].n_expanded == len(ref["expanded"])
        st, g, closed, opened = team.nodes(k)
        assert len(st) == ref["n_nodes"] == R[k].n_nodes
        cl = [chk.node(i)[3] for i in range(ref["n_nodes"])]
        op = [chk.node(i)[4] for i in range(ref["n_nodes"])]
        assert int(closed.sum()) == sum(cl)
        assert int(((opened == 1) & (closed == 0)).sum()) == sum(1 for a, b in zip(cl, op) if b and not a)
        for i in range(len(st)):
            s, gi = chk.node(i)[:2]
            assert np.array_equal(st[i][[0, 1, 2, 3, 4, 5, 12]], s[[0, 1, 2, 3, 4, 5, 12]]) and g[i] == gi, (k, i)
