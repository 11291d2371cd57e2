"""CPU: the point-cloud planner's CPU checker (tests/cloud_checker.py) against known answers -- the ellipsoid of a sample,
inside / outside points with and without the radius filter's truncation, the bounding box, the "every point is kept" rule,
empty and outlier clouds -- and the C-ABI handle's loud failure without a device."""
import ctypes as C
import math

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd.ellipsoid import control_lattice, state13
from oracle import orc
from tests import cloud_checker as K
from tests import cloud_scenes as S


def test_ellipsoid_at_rest_is_axis_aligned():
    Cm, (b1, b2, b3) = K.ellipsoid_C((0.5, 0.5, 0.1), (0.0, 0.0, 0.0))
    assert b3 == [0.0, 0.0, 1.0]
    assert np.allclose(Cm, np.diag([0.5, 0.5, 0.1]), rtol=0, atol=1e-15)
    ci = K.inverse3(Cm)
    assert np.allclose(ci, np.diag([2.0, 2.0, 10.0]), rtol=1e-15)


def test_ellipsoid_tilts_with_acceleration():
    _, (b1, b2, b3) = K.ellipsoid_C((0.5, 0.5, 0.1), (9.81, 0.0, 0.0))
    assert np.allclose(b3, np.array([1.0, 0.0, 1.0]) / math.sqrt(2), rtol=0, atol=1e-15)
    assert np.allclose(b2, [0.0, 1.0, 0.0], atol=1e-15)
    assert np.allclose(np.cross(b1, b2), b3, atol=1e-15)


def _prim(pos, vel, u, dt, control=orc.ACC):
    pr = orc.Primitive()
    w = orc.waypoint(pos, vel, control=control)
    orc.lib().orc_primitive_build(C.byref(w), (C.c_double * 3)(*u), dt, C.byref(pr))
    return pr


BOX = ((-5.0, -5.0, -5.0), (10.0, 10.0, 10.0))


def test_inside_and_outside_points():
    pr = _prim((0, 0, 0), (0, 0, 0), (0, 0, 0), 0.2)  # stationary: n = 0, the single sample t = 0 (E6)
    r = 0.5
    assert not K.Cloud([[0.0, 0.49, 0.0]], r, *BOX).is_free(pr, 0.2)
    assert K.Cloud([[0.0, 0.51, 0.0]], r, *BOX).is_free(pr, 0.2)
    assert not K.Cloud([[0.0, 0.0, 0.099]], r, *BOX).is_free(pr, 0.2)  # the height is 0.1
    assert K.Cloud([[0.0, 0.0, 0.101]], r, *BOX).is_free(pr, 0.2)


def test_radius_filter_truncates_a_flat_robot():
    """r = 0.05 < h = 0.1: a point inside E near its pole is outside the search radius, so it does not block"""
    pr = _prim((0, 0, 0), (0, 0, 0), (0, 0, 0), 0.2)
    r = 0.05
    pole = [[0.0, 0.0, 0.08]]
    Cm, _ = K.ellipsoid_C((r, r, 0.1), (0.0, 0.0, 0.0))
    assert K.inside(K.inverse3(Cm), [0.0, 0.0, 0.0], np.array(pole))[0]
    assert K.Cloud(pole, r, *BOX).is_free(pr, 0.2)
    assert not K.Cloud([[0.0, 0.0, 0.04]], r, *BOX).is_free(pr, 0.2)


def test_bounding_box_planes_and_samples():
    planes = K.bbox_planes((6.0, 12.0, 0.0), (25.0, 5.0, 1.5))
    assert [n for _, n in planes] == [(-1.0, -0.0, -0.0), (-0.0, -1.0, -0.0), (-0.0, -0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    assert planes[2][0] == (6.0 + 12.5, 12.0 + 0.75, 0.0)  # setBoundingBox's third point: ori + (dim.x / 2, dim.z / 2, 0)
    assert K.in_bbox(planes, (6.0, 12.0, 0.0)) and K.in_bbox(planes, (31.0, 17.0, 1.5))
    assert K.in_bbox(planes, (6.0 - 5e-11, 14.0, 1.0)) and not K.in_bbox(planes, (6.0 - 2e-10, 14.0, 1.0))
    cl = K.Cloud([], 0.5, (0, 0, 0), (1, 1, 1))
    assert cl.is_free(_prim((0.5, 0.5, 0.5), (0, 0, 0), (10, 0, 0), 0.2), 0.2)   # end x = 0.7
    assert not cl.is_free(_prim((0.5, 0.5, 0.5), (0, 0, 0), (40, 0, 0), 0.2), 0.2)  # end x = 1.3: outside


def test_every_point_is_kept_and_outliers_block():
    """setObstacles runs before setBoundingBox: a point outside the box still blocks a primitive near the edge"""
    pr = _prim((0.2, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 0.2)
    assert not K.Cloud([[-0.1, 0.5, 0.5]], 0.5, (0, 0, 0), (1, 1, 1)).is_free(pr, 0.2)
    far = K.Cloud([[-0.1, 0.5, 0.5], [1e4, -1e4, 3e3]], 0.5, (0, 0, 0), (1, 1, 1))
    assert not far.is_free(pr, 0.2)
    assert K.Cloud([[1e4, -1e4, 3e3]], 0.5, (0, 0, 0), (1, 1, 1)).is_free(pr, 0.2)
    assert K.Cloud(np.zeros((0, 3)), 0.5, (0, 0, 0), (1, 1, 1)).is_free(pr, 0.2)  # E7


def test_get_succ_skips_blocked_primitives():
    U = control_lattice(60.0, 2, False)
    assert len(U) == 25 and U[0].tolist() == [-60.0, -60.0, 0.0]
    assert len(control_lattice(60.0, 2, True, 1.0)) == 125
    cl = K.Cloud(S.office(), 0.5, S.ORI, S.DIM)
    ck = K.Checker(cl, orc.ACC, U, 0.2, v_max=10.0, a_max=10.0, w=10000.0)
    recs = ck.get_succ(state13((6.8, 13.0, 1.3)))
    assert any(not ok for ok, *_ in recs) and any(ok for ok, *_ in recs)
    for ok, st, cost, a in recs:
        assert math.isinf(cost) != ok
        assert st[12] == 0.2


def test_office_plan_on_the_checker():
    L = S.LAUNCH
    ck = K.Checker(K.Cloud(S.office(), L["r"], S.ORI, S.DIM), orc.ACC, control_lattice(L["u_max"], L["num"], False), L["dt"],
                   v_max=L["v_max"], a_max=L["a_max"], w=L["w"])
    r = ck.plan(state13(S.START), state13(S.GOAL), eps=L["eps"], tol_pos=2.0, tol_vel=2.0, tol_acc=100.0)
    assert r["status"] == 0 and r["traj"] is not None
    assert np.linalg.norm(r["traj"]["states"][-1, :3] - np.array(S.GOAL)) <= 2.0
    capped = ck.plan(state13(S.START), state13(S.GOAL), eps=L["eps"], tol_pos=2.0, tol_vel=2.0, tol_acc=100.0, max_num=10)
    assert capped["status"] == 3 and len(capped["expanded"]) == 10


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _capi.load()
    h = C.c_void_p()
    assert lib.mplx_cloud_create(0, C.byref(h)) == _capi.ERR_HIP
    assert b"HIP device" in lib.mplx_cloud_last_error(None)
    from mpl_ros_amd.ellipsoid import EllipsoidPlanner
    with pytest.raises(_capi.MplxError):
        EllipsoidPlanner()
