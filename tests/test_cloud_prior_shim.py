"""setPriorTrajectory through the C++ shim (include/mpl_shim/mpl_external_planner/ellipsoid_planner/ellipsoid_planner.h) and
tests/cpp/ellipsoid_prior_driver.cpp, which follows the prior-trajectory flow of ellipsoid_planner_node.cpp:63-163: an ACC
plan, setPriorTrajectory(getTraj()), the goal's use_acc / use_jrk cleared, a JRK plan.
CPU: header and driver compile; the driver links libmplx.so and fails loudly without a GPU.  GPU: the driver's costs,
expansion counts and guided trajectory equal the Python path's on the room of tests/test_cloud_prior.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import test_cloud_prior as T
from tests.test_ellipsoid_shim import HEADER, INC, LIBDIR, _has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "ellipsoid_prior_driver.cpp")
U_MAX, EPS, MAX_NUM, TOL = 2.5, 2.0, 2000, (2.0, 2.0, 100.0)  # (the node's setTol(2, 2, 100))


def build_driver(tmp_path):
    exe = str(tmp_path / "ellipsoid_prior_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall"] + INC + ["-o", exe, DRIVER, os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def driver_args(tmp_path):
    pts = T.room()
    path = str(tmp_path / "room.bin")
    pts.astype(np.float64).tofile(path)
    return [path, str(len(pts)), repr(T.R)] + [repr(float(x)) for x in T.ORI + T.DIM + T.START + T.GOAL] + \
        [repr(T.DT), repr(T.V_MAX), repr(T.A_MAX), repr(U_MAX), "1.0", "1", repr(T.W), repr(EPS), str(MAX_NUM), "0"]


def test_header_and_driver_compile():
    for src in (HEADER, DRIVER):
        subprocess.check_call(["g++", "-fsyntax-only", "-std=c++14", "-Wall", "-x", "c++"] + INC + [src])


def test_driver_fails_loudly_without_gpu(tmp_path):
    if _has_gpu():
        pytest.skip("GPU present")
    exe = build_driver(tmp_path)
    out = subprocess.run([exe] + driver_args(tmp_path), capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no HIP device" in out.stdout


@pytest.mark.gpu
def test_driver_equals_the_python_path(tmp_path):
    from mpl_ros_amd.ellipsoid import ACC, JRK, EllipsoidPlanner, control_lattice, prior_from_traj, state13
    exe = build_driver(tmp_path)
    out = subprocess.run([exe] + driver_args(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    d = json.loads(last[last.index("{"):])
    U = control_lattice(U_MAX, 1, False)
    pl = EllipsoidPlanner(False)
    pl.set_map(T.room(), T.R, T.ORI, T.DIM)
    pl.set_u(U)
    pl.set_dt(T.DT); pl.set_vmax(T.V_MAX); pl.set_amax(T.A_MAX); pl.set_w(T.W)
    pl.set_epsilon(EPS); pl.set_tol(*TOL); pl.set_max_num(MAX_NUM)
    pl.set_capacity(1, 1 << 20, 1 << 22, 1 << 21)
    start, goal = state13(T.START), state13(T.GOAL)
    pl.set_control(ACC)
    assert pl.plan(start, goal)
    r0, tr0 = pl.result(), pl.get_traj()
    assert d["prior_cost"] == r0["cost"] and d["prior_n_expanded"] == r0["n_expanded"] and d["prior_traj_len"] == r0["traj_len"]
    pl.set_prior_trajectory(prior_from_traj(tr0["states"], tr0["actions"], U, ACC, T.DT, T.W))
    pl.set_control(JRK)
    ok = pl.plan(start, goal)
    r = pl.result()
    assert ok and d["valid"] and d["status"] == r["status"] == 0
    assert d["cost"] == r["cost"] and d["n_expanded"] == r["n_expanded"] and d["traj_len"] == r["traj_len"] > 0
    tr = pl.get_traj()
    ws = np.array(d["traj"])
    assert ws.shape == (r["traj_len"] + 1, 13)
    # the waypoints at the joints are the stored states (the jerk of a joint is the segment's control input; the last
    # waypoint is evaluated by the host polynomial, not stored)
    assert np.array_equal(ws[:-1, :9], tr["states"][:-1, :9]) and np.array_equal(ws[:-1, 12], tr["states"][:-1, 12])
    assert np.array_equal(ws[:-1, 9:12], U[tr["actions"]])
    from mpl_ros_amd.ellipsoid import _poly
    s, u = tr["states"][-2], U[tr["actions"][-1]]
    end = [_poly([0.0, 0.0, float(u[k]), float(s[6 + k]), float(s[3 + k]), float(s[k])], T.DT) for k in range(3)]
    assert ws[-1, :12].tolist() == [end[k][d] for d in range(4) for k in range(3)]
    assert np.allclose(ws[-1, :9], tr["states"][-1, :9], rtol=0, atol=1e-9)
    # and the prior did guide the search
    pl.clear_prior_trajectory()
    assert pl.plan(start, goal) and pl.result()["expand_hash"] != r["expand_hash"]
