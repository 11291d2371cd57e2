"""The C++ side of the 3-D moving-obstacle planner: MPL::PolyMapPlanner3D of include/mpl_shim (poly_map_planner.h) and the
reference-free plumbing it plans through (poly3_device.h), driven by tests/cpp/poly_map_planner3d_driver.cpp and
tests/cpp/poly3_device_driver.cpp on the scene of tests/cpp/poly3_scene.h (SCENE below is the same scene in Python).
CPU: both drivers compile and fail loudly without a GPU; 3-D LPA* is refused.  GPU: the reference-free driver's plan equals
the Python path's."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mpl_ros_amd", "csrc")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "mpl_shim")]
REF_POLY = "/root/reference/mpl_external_planner/include"


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall"] + INC + list(extra) + ["-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                                                                                       os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def _has_gpu():
    import ctypes
    from mpl_ros_amd import _capi
    h = ctypes.c_void_p()
    if _capi.load().mplx_poly3_create(0, ctypes.byref(h)) == _capi.OK:
        _capi.load().mplx_poly3_destroy(h)
        return True
    return False


def _last_json(stdout):
    last = stdout.strip().splitlines()[-1]
    return json.loads(last[last.index("{"):])


def test_reference_free_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _build(tmp_path, "poly3_device_driver")
    if _has_gpu():
        pytest.skip("GPU present")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no HIP device" in out.stdout


@pytest.mark.skipif(not os.path.isdir(REF_POLY), reason="reference tree not present (GPU box)")
def test_poly_map_planner3d_compiles_against_the_reference_headers_and_refuses_lpastar(tmp_path):
    """MPL::PolyMapPlanner3D with include/mpl_shim AHEAD of the reference's include path (env_poly_map.h, poly_map_util.h,
    simple_obstacle.h stay the reference's): it compiles; without a GPU plan() fails loudly; setLPAstar(true), updateNodes()
    and getSubStateSpace() on a 3-D planner are refused, and nothing is planned on the CPU"""
    exe = _build(tmp_path, "poly_map_planner3d_driver", ["-I" + REF_POLY])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for what in ("setLPAstar(true) refused", "plan() with setLPAstar(true) refused", "updateNodes() refused", "getSubStateSpace() refused"):
        assert what in out.stdout
    r = _last_json(out.stdout)
    assert r["lpa_planned"] == 0
    if not _has_gpu():
        assert "no HIP device" in out.stdout and r["planned"] == 0 and r["traj_len"] == 0 and r["close_set"] == 0
    else:
        assert r["planned"] == 1 and r["traj_len"] > 0 and r["close_set"] > 0 and r["expanded_nodes"] > 0


def scene():
    """tests/cpp/poly3_scene.h in Python: (world, U, start, goal, planner set-up)"""
    from mpl_ros_amd import poly_map3d as p3
    s3 = 0.5773502691896258
    octa = np.array([[sx * 1.0, 0.0, 0.0, sx * s3, sy * s3, sz * s3] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    W = p3.PolyWorld3D((0.0, -5.0, 0.0), (10.0, 10.0, 4.0), start_t=0.5)
    W.static.append(p3.StaticObstacle3D(p3.box(0.8), (4.5, 0.5, 2.0)))
    W.static.append(p3.StaticObstacle3D(octa, (6.5, -2.0, 1.5)))
    W.linear.append(p3.LinearObstacle3D(p3.box(0.5), (6.0, 3.0, 2.0), (0.0, -0.5, 0.0), cov_v=0.1))
    segs = p3.acc_segs((3.0, -3.0, 2.0), (0.0, 0.0, 0.0), [(0, 1, 0), (0, 1, 0), (0, 0, 0), (0, 0, 0)], 0.5)
    W.nonlinear.append(p3.NonlinearObstacle3D(p3.box(0.5), segs, start_t=0.3, disappear_back=True))
    start, goal = np.zeros(13), np.zeros(13)
    start[0:3], start[12] = (1.0, 0.0, 2.0), 0.5
    goal[0:3] = (6.5, 1.0, 3.5)
    kw = dict(dt=0.5, v_max=2.0, a_max=1.5, j_max=-1.0, w=10.0)
    return W, p3.control_lattice(1.0, 1), start, goal, kw


@pytest.mark.gpu
def test_reference_free_driver_plan_equals_the_python_path(tmp_path):
    from mpl_ros_amd import poly_map3d as p3
    exe = _build(tmp_path, "poly3_device_driver")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = _last_json(out.stdout)
    W, U, start, goal, kw = scene()
    team = p3.PolyTeam3D()
    team.configure(p3.ACC, U, **kw)
    team.set_worlds([W])
    team.set_capacity(1, 1 << 20, 1 << 22, 1 << 21)
    r = team.plan_batch([0], [start], [goal], eps=1.0, tol_pos=0.5, max_expand=3000, heur_ignore_dynamics=False)[0]
    assert d["status"] == r.status == 0
    assert d["cost"] == r.cost and d["n_expanded"] == r.n_expanded and d["n_nodes"] == r.n_nodes and d["expanded"] == r.n_expanded
    act, ids, st = team.traj(0)
    assert d["actions"] == act.tolist() and len(act) > 0
    assert np.array_equal(np.array(d["states"]).reshape(-1, 13), st)  # the trajectory, state for state, bit for bit
    _, _, closed, _ = team.nodes(0)
    assert d["closed"] == int(closed.sum())
