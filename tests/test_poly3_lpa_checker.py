"""CPU: the checker the 3-D moving-obstacle LPA* (mplx_plpa3_*) is tested against (tests/cpp/poly_lpa_checker.cpp: the LPA* of
oracle/ref_stubs/poly_map_ref_api.cpp restated over the Env<Dim> of tests/cpp/poly_checker.cpp).

Dim 2 ties it to the reference: on the replanner flow of tests/test_poly_lpa.py it equals refpoly_lpa_* -- the LPA* over the COMPILED
reference environment -- bit for bit after every call.  Dim 3 is the same template on replanner_world3: against the checker's fresh
best-first search every tick, and the conditions the world was chosen for are asserted from the checker alone."""
import ctypes as C

import numpy as np
import pytest

from mpl_ros_amd import _capi
from mpl_ros_amd import poly_map as pm
from mpl_ros_amd import poly_map3d as p3
from oracle import refpoly
from tests import poly_lpa_checker as plc

KW = {pm.ACC: dict(dt=1.0, v_max=2.0, a_max=1.0, w=10.0), pm.JRK: dict(dt=1.0, v_max=2.0, a_max=1.0, j_max=1.0, w=10.0)}
CASES = [(pm.ACC, False), (pm.ACC, True), (pm.JRK, True)]  # (control, obstacles that change course)
KEYS = ("states", "g", "rhs", "h", "closed", "opened", "built", "child", "parent", "action", "blocked")


def same(sc, so, where):
    assert sc["initialized"] == so["initialized"] and sc["n_nodes"] == so["n_nodes"], where
    for k in KEYS:
        assert np.array_equal(sc[k], so[k]), (where, k)


@pytest.mark.skipif(not refpoly.available(), reason="oracle/_ref/libpolymap_ref.so not built (make -C oracle ref)")
@pytest.mark.parametrize("control,turn", CASES)
def test_dim2_lpastar_checker_equals_the_lpastar_over_the_compiled_reference(control, turn):
    R = refpoly.RefWorld(pm.replanner_world(0.0, turn), control, pm.U9, **KW[control])
    K = plc.LpaCheckerWorld(pm.replanner_world(0.0, turn), control, pm.U9, **KW[control])
    R.lpa_reset()
    start, goal = pm.replanner_endpoints()
    t, changes = 0.0, 0
    for tick in range(8):
        W = pm.replanner_world(t, turn)
        R.reload(W); K.reload(W)
        nb, nc = C.c_int(), C.c_int()
        R.L.refpoly_lpa_update_nodes(R.h, C.byref(nb), C.byref(nc))
        n = R.L.refpoly_lpa_num_changed()
        e = np.zeros(max(n, 1), dtype=np.int32); b = e.copy()
        R.L.refpoly_lpa_get_changed(e.ctypes.data, b.ctypes.data)
        uk = K.lpa_update_nodes()
        assert (nb.value, nc.value) == uk[:2], tick
        assert list(zip(e[:n].tolist(), b[:n].tolist())) == K.lpa_changed_raw(), tick   # the changed list, in the order of the walk
        changes += n
        same(K.lpa_state_space(), R.lpa_state_space(), (tick, "after updateNodes"))
        ro, rk = R.lpa_plan(start, goal), K.lpa_plan(start, goal)
        assert rk["status"] == ro["status"] and rk["cost"] == ro["cost"], tick
        for k in ("expanded", "actions", "node_ids"):
            assert np.array_equal(rk[k], ro[k]), (tick, k)
        same(K.lpa_state_space(), R.lpa_state_space(), (tick, "after plan"))
        if ro["status"] != 0 or len(ro["actions"]) <= 2:
            break
        ss = R.lpa_state_space()
        nid = ro["node_ids"][1]
        R.lpa_sub_state_space(1); K.lpa_sub_state_space(1)
        same(K.lpa_state_space(), R.lpa_state_space(), (tick, "after getSubStateSpace"))
        start = ss["states"][nid].copy()
        t += 1.0
        start[8] = t
    assert changes > 0 and tick >= 4


@pytest.mark.parametrize("control,turn", CASES)
def test_dim3_lpastar_checker_equals_its_fresh_search_on_replanner_world3(control, turn):
    """... and replanner_world3 is what it was chosen to be: a first plan of 50 to 5 000 expansions, entries that get cleared, with
    `turn` entries that get blocked, repairs that together expand fewer states than fresh plans."""
    K = plc.LpaCheckerWorld(p3.replanner_world3(0.0, turn), control, p3.U27, **KW[control])
    A = plc.LpaCheckerWorld(p3.replanner_world3(0.0, turn), control, p3.U27, **KW[control])
    assert len(p3.U27) == 27
    start, goal = p3.replanner_endpoints3()
    t, saw_blocked, saw_cleared, repairs = 0.0, 0, 0, []
    for tick in range(8):
        W = p3.replanner_world3(t, turn)
        assert W.dim[2] < W.dim[0] and all(o.cov_v > 0 for o in W.linear) and not W.static and not W.nonlinear
        K.reload(W); A.reload(W)
        nb, nc, ch = K.lpa_update_nodes()
        saw_blocked += nb; saw_cleared += nc
        assert len(ch) == nb + nc
        rl = K.lpa_plan(start, goal)
        ra = A.plan(start, goal)
        assert rl["status"] == ra["status"] and rl["cost"] == ra["cost"], tick
        repairs.append((len(rl["expanded"]), len(ra["expanded"])))
        if tick == 0:   # the first LPA* plan IS the best-first search: it expands the same states (ids differ -- the LPA* also keeps the
            sl = K.lpa_state_space()["states"][rl["expanded"]]   # successors whose primitive is blocked -- and with them the order among equal keys)
            sa = np.array([A.node(i)[0] for i in ra["expanded"]])
            cols = list(range(6)) + [12] if control == pm.ACC else list(range(9)) + [12]
            assert sorted(map(tuple, sl[:, cols])) == sorted(map(tuple, sa[:, cols]))
        if rl["status"] != 0 or len(rl["actions"]) <= 2:
            break
        ss = K.lpa_state_space()
        nid = rl["node_ids"][1]
        K.lpa_sub_state_space(1)
        start = ss["states"][nid].copy()
        t += 1.0
        start[12] = t
    assert len(repairs) == 8
    assert 50 <= repairs[0][0] <= 5000 and repairs[0][0] == repairs[0][1]
    assert saw_cleared > 0 and (saw_blocked > 0 or not turn)
    assert sum(l for l, a in repairs[1:]) < sum(a for l, a in repairs[1:])


def test_no_gpu_means_the_3d_lpastar_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = _capi.load()
    p = C.c_void_p()
    assert lib.mplx_poly3_create(0, C.byref(p)) == _capi.ERR_HIP and not p.value
    assert b"HIP device" in lib.mplx_poly3_last_error(None)
    l = C.c_void_p()
    assert lib.mplx_plpa3_create(p, C.byref(l)) == _capi.ERR_ARG and not l.value   # no handle to plan on: refused, never a silent planner
    assert b"mplx_poly3" in lib.mplx_plpa3_last_error(None)
    with pytest.raises(_capi.MplxError):
        p3.PolyTeam3D().lpa()
