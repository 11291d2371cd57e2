"""The C++ shim of the point-cloud planner (include/mpl_shim/mpl_external_planner/ellipsoid_planner/ellipsoid_planner.h) and
tests/cpp/ellipsoid_planner_driver.cpp, which repeats ellipsoid_planner_node.cpp:64-175 call for call.
CPU: header and driver compile; the driver links libmplx.so and fails loudly without a GPU; LPA* and prior trajectories
are refused.  GPU: the driver's status, cost, close-set size and trajectory length equal the Python path's."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cloud_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "mpl_ros_amd", "csrc")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "mpl_shim")]
HEADER = os.path.join(ROOT, "include", "mpl_shim", "mpl_external_planner", "ellipsoid_planner", "ellipsoid_planner.h")
DRIVER = os.path.join(ROOT, "tests", "cpp", "ellipsoid_planner_driver.cpp")


def build_driver(tmp_path):
    exe = str(tmp_path / "ellipsoid_planner_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall"] + INC + ["-o", exe, DRIVER, os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def driver_args(tmp_path, use_jrk=False, use_3d=False, max_num=-1):
    pts = S.office()
    path = str(tmp_path / "office.bin")
    pts.astype(np.float64).tofile(path)
    L = S.LAUNCH
    return [path, str(len(pts)), repr(L["r"])] + [repr(x) for x in S.ORI + S.DIM + S.START + S.GOAL] + \
        [repr(L["dt"]), repr(L["v_max"]), repr(L["a_max"]), repr(L["u_max"]), "1.0", str(L["num"]), repr(L["w"]), repr(L["eps"]),
         str(max_num), str(int(use_3d)), str(int(use_jrk))]


def _has_gpu():
    import ctypes
    from mpl_ros_amd import _capi
    h = ctypes.c_void_p()
    if _capi.load().mplx_cloud_create(0, ctypes.byref(h)) == _capi.OK:
        _capi.load().mplx_cloud_destroy(h)
        return True
    return False


def test_header_and_driver_compile():
    for src in (HEADER, DRIVER):
        subprocess.check_call(["g++", "-fsyntax-only", "-std=c++14", "-Wall", "-x", "c++"] + INC + [src])


def test_unsupported_requests_are_refused(tmp_path):
    """setLPAstar(true) and setPriorTrajectory make plan() fail with a message (before any device work)"""
    src = tmp_path / "refuse.cpp"
    src.write_text("""#include <mpl_external_planner/ellipsoid_planner/ellipsoid_planner.h>
int main() {
  Waypoint3D s(Control::ACC), g(Control::ACC);
  MPL::EllipsoidPlanner a(false);
  a.setLPAstar(true);
  const bool pa = a.plan(s, g);
  MPL::EllipsoidPlanner b(false);
  b.setPriorTrajectory(Trajectory<3>());
  const bool pb = b.plan(s, g);
  printf("%d %d %zu\\n", (int)pa, (int)pb, a.getExpandedNodes().size());
  return 0;
}
""")
    exe = str(tmp_path / "refuse")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall"] + INC + ["-o", exe, str(src), os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert "LPA* is not supported" in out.stdout and "prior trajectory" in out.stdout
    assert out.stdout.strip().splitlines()[-1].endswith("0 0 0")


def test_driver_fails_loudly_without_gpu(tmp_path):
    if _has_gpu():
        pytest.skip("GPU present")
    exe = build_driver(tmp_path)
    out = subprocess.run([exe] + driver_args(tmp_path), capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no HIP device" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("use_jrk", [False, True])
def test_driver_equals_the_python_path(tmp_path, use_jrk):
    """the node's start carries use_pos, use_vel, use_acc (launch default) and use_jrk: its control kind is JRK (states with
    acceleration), SNP with use_jrk"""
    from mpl_ros_amd.ellipsoid import JRK, SNP, EllipsoidPlanner, control_lattice, state13
    exe = build_driver(tmp_path)
    max_num = 3000 if use_jrk else -1
    out = subprocess.run([exe] + driver_args(tmp_path, use_jrk=use_jrk, max_num=max_num), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.strip().splitlines()[-1]
    d = json.loads(last[last.index("{"):])
    L = S.LAUNCH
    pl = EllipsoidPlanner(False)
    pl.set_map(S.office(), L["r"], S.ORI, S.DIM)
    pl.set_control(SNP if use_jrk else JRK)
    pl.set_u(control_lattice(L["u_max"], L["num"], False))
    pl.set_dt(L["dt"]); pl.set_vmax(L["v_max"]); pl.set_amax(L["a_max"]); pl.set_w(L["w"])
    pl.set_epsilon(L["eps"]); pl.set_tol(*L["tol"]); pl.set_max_num(max_num)
    pl.set_capacity(1, 1 << 20, 1 << 22, 1 << 21)
    ok = pl.plan(state13(S.START), state13(S.GOAL))
    r = pl.result()
    assert d["status"] == r["status"] and d["valid"] == ok
    assert d["cost"] == r["cost"]
    assert d["close_set"] == len(pl.get_close_set()) and d["open_set"] == len(pl.get_open_set())
    assert d["n_expanded"] == r["n_expanded"] and d["expanded_nodes"] == 0
    assert d["traj_len"] == (r["traj_len"] if ok else 0)
    if not use_jrk:
        assert ok and d["traj_len"] > 0
