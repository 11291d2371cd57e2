"""The C++ side of the 3-D moving-obstacle planner's state space: getValidPrimitives / getAllPrimitives of MPL::PolyMapPlanner3D
(include/mpl_shim, poly_map_planner.h) and the reference-free plumbing they read through (poly3_device.h: poly3_space_fetch),
driven by tests/cpp/poly3_space_driver.cpp on the scene of tests/cpp/poly3_scene.h (tests/test_poly_map3d_shim.py: scene() is the
same scene in Python).  The driver has two builds that print the same line: the planner itself where the reference's
poly_map_planner headers are present, the reference-free plumbing everywhere.  CPU: both builds compile and fail loudly without a
GPU.  GPU: sizes, first and last primitive and a digest of all coefficients against the CPU checker's space; the refusals."""
import os
import subprocess

import numpy as np
import pytest

from mpl_ros_amd import poly_map3d as p3
from tests.poly_space_checker import SpaceChecker
from tests.test_poly_map3d_shim import INC, LIBDIR, REF_POLY, ROOT, _has_gpu, _last_json, scene

PLAN_KW = dict(eps=1.0, tol_pos=0.5, max_expand=3000, heur_ignore_dynamics=False)  # (poly3_scene.h: EPS, TOL_POS, MAX_NUM)
NOT_PLANNED = "refused: this PolyMapPlanner3D has not planned on the device"
REPLACED = "another planner has planned on the shared device object"


# the planner build compiles the reference's headers: a reference binary, it lives in oracle/_ref/ with the other ones
PLANNER_BIN = os.path.join(ROOT, "oracle", "_ref", "poly3_space_driver_planner")
SRC = os.path.join(ROOT, "tests", "cpp", "poly3_space_driver.cpp")


def build_planner_driver():
    """tests/cpp/poly3_space_driver.cpp with -DPOLY3_SPACE_WITH_PLANNER: MPL::PolyMapPlanner3D with include/mpl_shim AHEAD of the
    reference's include path.  Needs the reference tree: done where it is present (__graft_entry__.build()); a machine without it
    runs the prebuilt binary (it travels like the .so files)."""
    os.makedirs(os.path.dirname(PLANNER_BIN), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-DPOLY3_SPACE_WITH_PLANNER"] + INC + ["-I" + REF_POLY, "-o", PLANNER_BIN, SRC, "-L" + LIBDIR, "-lmplx",
                                                                                                      "-Wl,-rpath,$ORIGIN/../../mpl_ros_amd/csrc"])


def _build(tmp_path, with_planner):
    if with_planner:
        if os.path.isdir(REF_POLY):
            build_planner_driver()
        return PLANNER_BIN
    exe = str(tmp_path / "poly3_space_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall"] + INC + ["-o", exe, SRC, os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


# the reference-free build everywhere; the planner build where the reference's headers are, or where it has been prebuilt
BUILDS = [False] + ([True] if os.path.isdir(REF_POLY) or os.path.exists(PLANNER_BIN) else [])


@pytest.mark.parametrize("with_planner", BUILDS)
def test_driver_compiles_and_fails_loudly_without_gpu(tmp_path, with_planner):
    exe = _build(tmp_path, with_planner)
    if _has_gpu():
        return  # (the GPU test below runs it)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "no HIP device" in out.stdout
    # the never-planned planner was refused -- before anything touched the device -- and nothing is served
    assert out.stdout.index(NOT_PLANNED) < out.stdout.index("no HIP device")
    assert "getValidPrimitives() " + NOT_PLANNED in out.stdout and "getAllPrimitives() " + NOT_PLANNED in out.stdout
    r = _last_json(out.stdout)
    assert r["planned"] == 0 and r["sizes"] == [0, 0, 0, 0, 0] and r["never"] == [0, 0] and r["after_other"] == [0, 0]


_ref = {}


def checker_space():
    """the checker's space of the scene's plan: (result, space, blocked, coefficients of every record's primitive, valid ones first)"""
    if not _ref:
        W, U, start, goal, env = scene()
        chk = SpaceChecker(W, p3.ACC, U, **env)
        r = chk.plan(start, goal, **PLAN_KW)
        sp, bl = chk.space(), chk.blocked()
        parent = np.concatenate([sp["parent"], bl[0]])
        action = np.concatenate([sp["action"], bl[1]])
        c = np.zeros((len(parent), 3, 6))  # Primitive(parent state, U[action], dt) of an ACC state: {0, 0, 0, u, vel, pos} per axis
        c[:, :, 3] = U[action]
        c[:, :, 4] = sp["states"][parent][:, 3:6]
        c[:, :, 5] = sp["states"][parent][:, 0:3]
        _ref.update(r=r, sp=sp, bl=bl, c=c)
    return _ref["r"], _ref["sp"], _ref["bl"], _ref["c"]


def test_scene_has_valid_and_blocked_records_and_an_open_frontier():
    r, sp, bl, c = checker_space()
    assert r["status"] == 0 and len(sp["child"]) > 0 and len(bl[0]) > 0 and len(c) == len(sp["child"]) + len(bl[0])
    assert np.sum(sp["closed"] != 0) > 0 and np.sum((sp["opened"] != 0) & (sp["closed"] == 0)) > 0


def digest(c):
    """poly3_space_driver.cpp: sum of bit pattern x (index + 1) over the coefficients, modulo 2^64"""
    bits = np.ascontiguousarray(c, dtype=np.float64).reshape(-1).view(np.uint64)
    with np.errstate(over="ignore"):
        return int((bits * np.arange(1, len(bits) + 1, dtype=np.uint64)).sum(dtype=np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("with_planner", BUILDS)
def test_getter_sizes_and_primitives_equal_the_checker_space(tmp_path, with_planner):
    exe = _build(tmp_path, with_planner)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = _last_json(out.stdout)
    r, sp, bl, c = checker_space()
    n_closed, n_open = int(np.sum(sp["closed"] != 0)), int(np.sum((sp["opened"] != 0) & (sp["closed"] == 0)))
    assert d["planned"] == 1 and d["status"] == r["status"] == 0
    assert d["sizes"] == [n_closed, n_open, len(r["expanded"]), len(sp["child"]), len(sp["child"]) + len(bl[0])]
    assert np.array_equal(np.array(d["first"]), c[0].reshape(-1)) and np.array_equal(np.array(d["last"]), c[-1].reshape(-1))
    assert int(d["digest"]) == digest(c)
    # a second planner has planned on the shared device object: the first one's primitives are refused, nothing is served
    assert d["other_planned"] == 1 and d["after_other"] == [0, 0] and REPLACED in out.stdout
    # a planner that never planned: refused, empty
    assert d["never"] == [0, 0] and "getValidPrimitives() " + NOT_PLANNED in out.stdout and "getAllPrimitives() " + NOT_PLANNED in out.stdout
