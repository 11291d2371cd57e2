"""getValidPrimitives / getAllPrimitives of the C++ shim of the point-cloud planner (include/mpl_shim/mpl_external_planner/
ellipsoid_planner/ellipsoid_planner.h), served from the device's state-space export, through tests/cpp/ellipsoid_space_driver.cpp.
CPU: header and driver compile; without a GPU plan() fails and both getters are empty.  GPU: the number of primitives equals the plan's
n_edges and their digest equals the one computed here from EllipsoidPlanner.state_space() and the lattice; the two getters agree."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import cloud_scenes as S
from tests.test_ellipsoid_shim import HEADER, INC, LIBDIR, _has_gpu, driver_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "ellipsoid_space_driver.cpp")
MAX_NUM = 200


def build_driver(tmp_path):
    exe = str(tmp_path / "ellipsoid_space_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall"] + INC + ["-o", exe, DRIVER, os.path.join(LIBDIR, "libmplx.so"), "-Wl,-rpath," + LIBDIR])
    return exe


def run_driver(tmp_path, **kw):
    out = subprocess.run([build_driver(tmp_path)] + driver_args(tmp_path, **kw), capture_output=True, text=True, timeout=120)
    last = out.stdout.strip().splitlines()[-1]
    return out, json.loads(last[last.index("{"):])


def fnv1a(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def coefficients(states, parent, action, U, control):
    """Primitive<3>(parent state, U[action], dt) of every record: m x 3 x 6 coefficients (mpl_basis/primitive.h: the control input in the
    column of its derivative, the state's derivatives behind it, zeros in front)"""
    kind = {1: 1, 3: 2, 7: 3, 15: 4}[control]  # VEL ACC JRK SNP: order of the derivative the input sets
    m = len(parent)
    co = np.zeros((m, 3, 6))
    st = states[parent]
    co[:, :, 5 - kind] = U[action]
    for d in range(kind):  # pos, vel, acc, jrk
        co[:, :, 5 - d] = st[:, 3 * d:3 * d + 3]
    return co


def test_header_and_driver_compile():
    for src in (HEADER, DRIVER):
        subprocess.check_call(["g++", "-fsyntax-only", "-std=c++14", "-Wall", "-x", "c++"] + INC + [src])


def test_without_a_gpu_plan_fails_and_both_getters_are_empty(tmp_path):
    if _has_gpu():
        pytest.skip("GPU present")
    out, d = run_driver(tmp_path, max_num=MAX_NUM)
    assert out.returncode == 3 and "no HIP device" in out.stdout
    assert not d["ran"] and not d["valid"]
    assert d["before_valid"] == d["before_all"] == d["valid_primitives"] == d["all_primitives"] == 0
    assert d["valid_digest"] == d["all_digest"] == f"{fnv1a(b''):016x}"


@pytest.mark.gpu
@pytest.mark.parametrize("use_jrk", [False, True])
def test_primitives_equal_the_python_state_space(tmp_path, use_jrk):
    from mpl_ros_amd.ellipsoid import JRK, SNP, EllipsoidPlanner, control_lattice, state13
    out, d = run_driver(tmp_path, use_jrk=use_jrk, max_num=MAX_NUM)
    assert out.returncode == 0, out.stdout + out.stderr
    L = S.LAUNCH
    control = SNP if use_jrk else JRK
    U = control_lattice(L["u_max"], L["num"], False)
    pl = EllipsoidPlanner(False)
    pl.set_map(S.office(), L["r"], S.ORI, S.DIM)
    pl.set_control(control)
    pl.set_u(U)
    pl.set_dt(L["dt"]); pl.set_vmax(L["v_max"]); pl.set_amax(L["a_max"]); pl.set_w(L["w"])
    pl.set_epsilon(L["eps"]); pl.set_tol(*L["tol"]); pl.set_max_num(MAX_NUM)
    pl.set_capacity(1, 1 << 20, 1 << 22, 1 << 21)
    ok = pl.plan(state13(S.START), state13(S.GOAL))
    r = pl.result()
    assert d["ran"] and d["valid"] == ok and d["status"] == r["status"] and d["n_nodes"] == r["n_nodes"] and d["n_edges"] == r["n_edges"]
    assert d["before_valid"] == d["before_all"] == 0
    assert d["valid_primitives"] == d["all_primitives"] == r["n_edges"] > 100
    assert d["t"] == L["dt"]  # (the dt of the plan, not the one set afterwards)
    ss = pl.state_space(0)
    co = coefficients(ss["states"], ss["parent"], ss["action"], U, control)
    want = f"{fnv1a(np.ascontiguousarray(co, dtype='<f8').tobytes()):016x}"
    assert d["valid_digest"] == d["all_digest"] == want
