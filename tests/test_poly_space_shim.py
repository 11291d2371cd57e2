"""The C++ side of the 2-D moving-obstacle planner's state space: the five getters of MPL::PolyMapPlanner2D (include/mpl_shim,
poly_map_planner.h) and the reference-free plumbing they read through (poly2_space.h), driven by
tests/cpp/poly_map_getters_driver.cpp and tests/cpp/poly2_space_driver.cpp on the replanner flow's world (scene() below is the
same scene in Python).  CPU: both drivers compile; without a GPU they refuse loudly and every set is empty.  GPU: the
reference-free driver's sets equal PolyTeam's; after another plan on the shared object they are refused; in LPA* mode the
getters' sizes equal the counts of the mplx_plpa_result_* entries."""
import json
import os
import subprocess

import numpy as np
import pytest

from mpl_ros_amd import poly_map as pm

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
    if _capi.load().mplx_poly_create(0, ctypes.byref(h)) == _capi.OK:
        _capi.load().mplx_poly_destroy(h)
        return True
    return False


def _last_json(stdout):
    last = stdout.strip().splitlines()[-1]
    return json.loads(last[last.index("{"):])


def test_reference_free_driver_compiles_and_fails_loudly_without_gpu(tmp_path):
    exe = _build(tmp_path, "poly2_space_driver")
    if _has_gpu():
        return  # (the GPU tests below run it)
    for args in ([], ["lpa"]):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 3 and "no HIP device" in out.stdout


@pytest.mark.skipif(not os.path.isdir(REF_POLY), reason="reference tree not present (GPU box)")
def test_getters_driver_compiles_against_the_reference_headers(tmp_path):
    """MPL::PolyMapPlanner2D / 3D with include/mpl_shim AHEAD of the reference's include path: the five getters in A* mode, with
    setLPAstar(true), through a PlannerBase reference and on a 3-D planner.  Without a GPU the planners refuse and every set
    is empty; the 3-D primitives are refused with a message either way."""
    exe = _build(tmp_path, "poly_map_getters_driver", ["-I" + REF_POLY])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    r = _last_json(out.stdout)
    assert "getValidPrimitives() refused" in out.stdout and "getAllPrimitives() refused" in out.stdout and r["valid3"] == 0 and r["all3"] == 0
    assert r["before_plan"] == [0, 0, 0, 0, 0]
    if not _has_gpu():
        assert "no HIP device" in out.stdout and r["planned"] == [0, 0, 0]
        for k in ("astar", "astar_base", "lpa", "astar_after_lpa", "other", "astar_after_other"):
            assert r[k] == [0, 0, 0, 0, 0], k
    else:
        assert r["planned"] == [1, 1, 1]
        assert min(r["astar"]) > 0 and r["astar_base"] == r["astar"] == r["astar_after_lpa"] and r["astar"][4] >= r["astar"][3]
        assert min(r["lpa"]) > 0 and min(r["other"]) > 0
        assert r["astar_after_other"] == [0, 0, 0, 0, 0] and "another planner has planned on the shared device object" in out.stdout


def scene(t=0.0):
    """tests/cpp/poly2_space_driver.cpp in Python: (world at time t, U, start, goal, set-up, plan arguments)"""
    W = pm.replanner_world(t)
    assert len(W.linear) == 5 and np.array_equal(W.dim, (20.0, 20.0))
    start, goal = pm.replanner_endpoints()
    env = dict(dt=1.0, v_max=2.0, a_max=1.0, j_max=-1.0, w=10.0)
    kw = dict(eps=1.0, tol_pos=0.5, max_expand=2000, heur_ignore_dynamics=True)
    return W, pm.U9, start, goal, env, kw


@pytest.mark.gpu
def test_reference_free_driver_sets_equal_the_python_path_and_are_refused_after_another_plan(tmp_path):
    exe = _build(tmp_path, "poly2_space_driver")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = _last_json(out.stdout)
    W, U, start, goal, env, kw = scene()
    team = pm.PolyTeam()
    team.configure(pm.ACC, U, **env)
    team.set_worlds([W])
    team.set_capacity(1, 1 << 20, 1 << 22, 1 << 21)
    team.set_record(1 << 20)
    r = team.plan_batch([0], [start], [goal], **kw)[0]
    sp = team.state_space(0)
    assert d["status"] == r.status and d["n_nodes"] == r.n_nodes == sp["n_nodes"] and d["n_expanded"] == r.n_expanded and r.n_nodes > 0
    close, opn = team.close_set(0), team.open_set(0)
    assert len(close) > 0 and len(opn) > 0
    assert np.array_equal(np.array(d["close_set"]).reshape(-1, 2), close)
    assert np.array_equal(np.array(d["open_set"]).reshape(-1, 2), opn)
    assert np.array_equal(np.array(d["expanded_nodes"]).reshape(-1, 2), sp["states"][team.expanded_ids(0)][:, 0:2]) and len(d["expanded_nodes"]) == 2 * r.n_expanded
    n_blocked = len(team.blocked(0)[0])
    assert d["valid"] == d["valid_first"] == len(sp["child"]) > 0 and d["all"] == len(sp["child"]) + n_blocked and n_blocked > 0
    # the second plan on the shared object: the first planner's getters print the refusal and return empty
    assert d["served_after_other_plan"] == 0 and "another planner has planned on the shared device object" in out.stdout
    assert [d[k] for k in ("after_close", "after_open", "after_expanded", "after_valid", "after_all")] == [0, 0, 0, 0, 0]


@pytest.mark.gpu
def test_lpa_mode_getter_sizes_equal_the_entry_counts_over_three_ticks(tmp_path):
    exe = _build(tmp_path, "poly2_space_driver")
    out = subprocess.run([exe, "lpa"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ticks = _last_json(out.stdout)["ticks"]
    assert len(ticks) == 3
    for k, t in enumerate(ticks):
        assert t["status"] == 0, (k, t)
        assert t["getters"] == t["counts"] and min(t["counts"][0:2]) > 0 and t["counts"][4] >= t["counts"][3] > 0, (k, t)
    assert ticks[0]["counts"][2] > 0 and any(t["counts"][4] > t["counts"][3] for t in ticks)  # (an expansion record; blocked entries exist)
