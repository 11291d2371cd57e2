"""The state space of the moving-obstacle LPA* planners exported on the device (mplx_plpa_export_* / mplx_plpa3_export_*;
PolyLpa.space / records / changed_primitives, PolyLpaFleet.spaces and their 3-D twins): passes over the handles' pools instead of two
pool copies decoded on the host.  Everything is bit-exact, no tolerance anywhere: after every call of the replanner flow space() equals
the CPU LPA* checker (tests/poly_lpa_checker.py, Dim 2 and 3 -- tests/test_poly3_lpa_checker.py pins it to the compiled reference) and
the host-decoded state_space() on every key; states are keyed on the control's columns as in tests/test_poly3_lpa.py.

CPU: the symbols load; NULL handles, NULL arrays, NULL entries and arrays that mix planner objects are refused with MPLX_ERR_ARG
without touching a device; an array of handles that never planned counts 0.  GPU: the replanner flow, a size sweep across the tile
(256) and the scan chunk (256 tiles = 65 536 entries), the record filter, the changed primitives, empty spaces and small caps, arrays
of handles (a fleet's members)."""
import ctypes as C

import numpy as np
import pytest

from mpl_ros_amd import _capi, plpa_space
from mpl_ros_amd import poly_map as pm
from mpl_ros_amd import poly_map3d as p3
from mpl_ros_amd._capi import MplxError
from tests import poly_lpa_checker as plc

ACC, JRK = pm.ACC, pm.JRK
assert (p3.ACC, p3.JRK) == (ACC, JRK)
KW = {ACC: dict(dt=1.0, v_max=2.0, a_max=1.0, w=10.0), JRK: dict(dt=1.0, v_max=2.0, a_max=1.0, j_max=1.0, w=10.0)}
KEYS = ("states", "g", "rhs", "h", "closed", "opened", "built", "child", "parent", "action", "blocked")
TILE = 256
SENTINEL_I, SENTINEL_D = -77, -7.25


class Dim:
    def __init__(self, dim):
        self.dim = dim
        self.mod = pm if dim == 2 else p3
        self.prefix = "plpa" if dim == 2 else "plpa3"
        self.W = 9 if dim == 2 else 13
        self.U = pm.U9 if dim == 2 else p3.U27
        self.world = pm.replanner_world if dim == 2 else p3.replanner_world3
        self.endpoints = pm.replanner_endpoints if dim == 2 else p3.replanner_endpoints3
        # what a state is keyed on -- ACC: pos vel t, JRK: + acc (the checker's Waypoint also carries the control input it arrived with)
        self.cols = {ACC: list(range(2 * dim)) + [self.W - 1], JRK: list(range(3 * dim)) + [self.W - 1]}

    def team(self, control, worlds, U=None):
        t = self.mod.PolyTeam() if self.dim == 2 else self.mod.PolyTeam3D()
        t.configure(control, self.U if U is None else U, **KW[control])
        t.set_worlds(worlds)
        t.set_capacity(1, 1 << 16, 1 << 19, 1 << 19)
        return t

    def pair(self, control, turn=True, U=None, cap=(1 << 16, 1 << 20, 1 << 20)):
        """(checker, team, planner) on the replanner world at t = 0"""
        W = self.world(0.0, turn)
        K = plc.LpaCheckerWorld(W, control, self.U if U is None else U, **KW[control])
        team = self.team(control, [W], U)
        l = team.lpa()
        l.set_capacity(*cap)
        return K, team, l

    def fn(self, lib, name):
        return getattr(lib, "mplx_%s_export_%s" % (self.prefix, name))


DIMS = {2: Dim(2), 3: Dim(3)}


def same(a, b, cols=None, where=""):
    """two state-space dicts, key for key (states on `cols` when given)"""
    assert a["initialized"] == b["initialized"], where
    assert a["n_nodes"] == b["n_nodes"], where
    for k in KEYS:
        x, y = (a[k][:, cols], b[k][:, cols]) if k == "states" and cols is not None else (a[k], b[k])
        assert x.shape == y.shape and np.array_equal(x, y), (where, k)


def check_space(D, K, l, control, where=""):
    """space() == the checker's space == state_space(), on every key"""
    sx, sh, so = l.space(), l.state_space(), K.lpa_state_space()
    same(sx, sh, None, (where, "export against the host-decoded dump"))
    assert sx["initialized"] == so["initialized"], where
    if so["initialized"]:
        same(sx, so, D.cols[control], (where, "export against the checker"))
    else:
        assert sx["n_nodes"] == 0 and len(sx["child"]) == 0, where
    return sx


def check_records(l, sx, where=""):
    """records(1) followed by records(2) is records(0) split by its blocked column, order kept; entry indexes records(0)"""
    r0, r1, r2 = l.records(0), l.records(1), l.records(2)
    m = len(sx["child"])
    assert np.array_equal(r0["entry"], np.arange(m)), where
    for k in ("child", "parent", "action", "blocked"):
        assert np.array_equal(r0[k], sx[k]), (where, k)
    b = r0["blocked"] != 0
    for r, sel, bit in ((r1, ~b, 0), (r2, b, 1)):
        assert np.array_equal(r["entry"], np.nonzero(sel)[0]), where
        assert np.all(r["blocked"] == bit), where
        for k in ("child", "parent", "action", "blocked"):
            assert np.array_equal(r[k], r0[k][sel]) and np.array_equal(r[k], r0[k][r["entry"]]), (where, k)
    return int(b.sum())


def check_changed(l, sx, where=""):
    """changed_primitives() rows are states[parent[e]], action[e] and the now-blocked bit for every e of changed()"""
    ch = l.changed()
    rows, action, now = l.changed_primitives()
    assert len(rows) == len(action) == len(now) == len(ch), where
    if ch:
        e = np.array([c[0] for c in ch])
        assert np.array_equal(rows, sx["states"][sx["parent"][e]]), where
        assert np.array_equal(action, sx["action"][e]) and np.array_equal(now, np.array([c[1] for c in ch])), where
        assert np.array_equal(now, sx["blocked"][e]), where  # (the bit the entry carries now)
    return len(ch)


# ---------------------------------------------------------------------------------------------------------------- CPU
NAMES = ["space", "records", "changed", "ms", "space_many", "records_many"]


def test_library_exports_the_state_space_exports_and_capi_binds_them():
    lib = _capi.load()
    for prefix in ("plpa", "plpa3"):
        for n in NAMES:
            name = "mplx_%s_export_%s" % (prefix, n)
            assert name in _capi.EXPORTS
            assert getattr(lib, name) is not None
    assert "mplx_plpa_export_last_error" in _capi.EXPORTS and lib.mplx_plpa_export_last_error() is not None


@pytest.mark.parametrize("dim", [2, 3])
def test_null_handles_and_null_arrays_are_refused_without_touching_a_device(dim):
    D, lib = DIMS[dim], _capi.load()
    n = C.c_uint64(99)
    a = np.full(8, SENTINEL_I, dtype=np.int32)
    d = np.full(8 * D.W, SENTINEL_D)
    assert D.fn(lib, "space")(None, 8, d.ctypes.data, None, None, None, a.ctypes.data, None, None, C.byref(n)) == _capi.ERR_ARG and n.value == 0
    assert b"handle 0 is NULL" in lib.mplx_plpa_export_last_error()
    n.value = 99
    assert D.fn(lib, "records")(None, 0, 8, a.ctypes.data, None, None, None, None, C.byref(n)) == _capi.ERR_ARG and n.value == 0
    n.value = 99
    assert D.fn(lib, "changed")(None, 8, d.ctypes.data, a.ctypes.data, None, C.byref(n)) == _capi.ERR_ARG and n.value == 0
    ms = (C.c_float * 3)()
    assert D.fn(lib, "ms")(None, ms) == _capi.ERR_ARG
    off = np.full(3, 99, dtype=np.uint64)
    assert D.fn(lib, "space_many")(2, None, 8, off.ctypes.data, d.ctypes.data, None, None, None, None, None, None) == _capi.ERR_ARG
    assert D.fn(lib, "records_many")(2, None, 0, 8, off.ctypes.data, a.ctypes.data, None, None, None, None) == _capi.ERR_ARG
    arr = (C.c_void_p * 2)(None, None)
    assert D.fn(lib, "space_many")(0, arr, 8, off.ctypes.data, d.ctypes.data, None, None, None, None, None, None) == _capi.ERR_ARG
    assert D.fn(lib, "space_many")(2, arr, 8, off.ctypes.data, d.ctypes.data, None, None, None, None, None, None) == _capi.ERR_ARG
    assert b"handle 0 is NULL" in lib.mplx_plpa_export_last_error()
    assert np.all(a == SENTINEL_I) and np.all(d == SENTINEL_D)


@pytest.mark.parametrize("dim", [2, 3])
def test_arrays_that_mix_planner_objects_are_refused_and_unplanned_handles_count_zero(dim):
    """mplx_plpa_create / mplx_plpa3_create do no device work and only keep the object pointer, so two stand-in objects do for the
    check that comes before any launch; the handles never plan."""
    D, lib = DIMS[dim], _capi.load()
    create, destroy, last_error = (getattr(lib, "mplx_%s_%s" % (D.prefix, n)) for n in ("create", "destroy", "last_error"))
    objs = [C.create_string_buffer(64), C.create_string_buffer(64)]
    hs = []
    for o in (objs[0], objs[0], objs[1]):
        h = C.c_void_p()
        assert create(C.cast(o, C.c_void_p), C.byref(h)) == _capi.OK and h.value
        hs.append(h)
    try:
        off = np.full(4, 99, dtype=np.uint64)
        a = np.full(8, SENTINEL_I, dtype=np.int32)
        d = np.full(8 * D.W, SENTINEL_D)
        mixed = (C.c_void_p * 3)(*[h.value for h in hs])
        for call in (lambda: D.fn(lib, "space_many")(3, mixed, 8, off.ctypes.data, d.ctypes.data, None, None, None, a.ctypes.data, None, None),
                     lambda: D.fn(lib, "records_many")(3, mixed, 0, 8, off.ctypes.data, a.ctypes.data, a.ctypes.data, None, None, None)):
            assert call() == _capi.ERR_ARG
            assert b"handle 2 is bound to another" in lib.mplx_plpa_export_last_error()
            assert b"handle 2 is bound to another" in last_error(hs[0])
        holed = (C.c_void_p * 3)(hs[0].value, None, hs[1].value)
        assert D.fn(lib, "space_many")(3, holed, 8, off.ctypes.data, d.ctypes.data, None, None, None, None, None, None) == _capi.ERR_ARG
        assert b"handle 1 is NULL" in last_error(hs[1])
        # handles on one object that never planned: nothing to serve, no device needed
        alike = (C.c_void_p * 2)(hs[0].value, hs[1].value)
        assert D.fn(lib, "space_many")(2, alike, 0, off.ctypes.data, d.ctypes.data, None, None, None, a.ctypes.data, None, None) == _capi.OK
        assert off[:3].tolist() == [0, 0, 0]
        off[:] = 99
        assert D.fn(lib, "records_many")(2, alike, 2, 8, off.ctypes.data, a.ctypes.data, None, None, None, None) == _capi.OK
        assert off[:3].tolist() == [0, 0, 0]
        assert D.fn(lib, "records_many")(2, alike, 3, 8, off.ctypes.data, a.ctypes.data, None, None, None, None) == _capi.ERR_ARG  # which
        n = C.c_uint64(99)
        assert D.fn(lib, "changed")(hs[0], 8, d.ctypes.data, a.ctypes.data, a.ctypes.data, C.byref(n)) == _capi.OK and n.value == 0
        ms = (C.c_float * 3)(1, 1, 1)
        assert D.fn(lib, "ms")(hs[0], ms) == _capi.OK and list(ms) == [0, 0, 0]
        assert np.all(a == SENTINEL_I) and np.all(d == SENTINEL_D)
    finally:
        for h in hs:
            destroy(h)


def test_without_a_gpu_the_planner_object_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(MplxError):
        pm.PolyTeam()
    with pytest.raises(MplxError):
        p3.PolyTeam3D()


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("dim,control,ticks", [(2, ACC, 3), (3, ACC, 3), (3, JRK, 1)])
def test_space_equals_the_checker_and_the_host_dump_after_every_call_of_the_replanner_flow(dim, control, ticks):
    D = DIMS[dim]
    K, team, l = D.pair(control)
    start, goal = D.endpoints()
    t = 0.0
    for tick in range(ticks):
        W = D.world(t, True)
        K.reload(W)
        team.set_worlds([W])
        uo, ud = K.lpa_update_nodes(), l.update_nodes()
        assert ud == uo, (tick, ud[:2], uo[:2])
        sx = check_space(D, K, l, control, (tick, "update"))
        assert check_changed(l, sx, (tick, "update")) == len(uo[2])
        ro, ok = K.lpa_plan(start, goal), l.plan(start, goal)
        assert l.result.status == ro["status"] == 0 and ok and len(ro["actions"]) > 2, tick
        sx = check_space(D, K, l, control, (tick, "plan"))
        check_records(l, sx, (tick, "plan"))
        act, ids, st = l.traj()
        K.lpa_sub_state_space(1)
        l.sub_state_space(1)
        check_space(D, K, l, control, (tick, "re-root"))
        start = st[1].copy()
        t += 1.0
        start[D.W - 1] = t


# first plans capped with max_expand: (lattice, cap, start -> goal or None for the replanner endpoints)
U5 = np.array([(0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)])
U7 = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)])
SWEEP = {2: [(U5, 1, None), (None, 20, None), (None, 100, None)],
         3: [(U7, 1, None), (None, 8, None), (None, 60, None), (None, -1, ((18.0, 12.0, 2.0), (3.0, 8.0, 2.0)))]}


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_size_sweep_across_the_tile_and_the_scan_chunk(dim):
    """The tile (256 states / entries) and the scan chunk (256 tiles) are the only places the passes can go wrong: the spaces, sized
    with the CPU checker, are a single-digit one, one below a tile, one above a tile that is no multiple of it and (3-D) one above
    65 536 entries; the root has no predecessor, some state has more than one."""
    D = DIMS[dim]
    sizes, multi = [], False
    for U, cap, ends in SWEEP[dim]:
        K, team, l = D.pair(ACC, U=U, cap=(1 << 17, 1 << 20, 1 << 20))
        start, goal = D.endpoints()
        if ends is not None:
            start[:3], goal[:3] = ends
        ro, ok = K.lpa_plan(start, goal, max_expand=cap), l.plan(start, goal, max_expand=cap)
        assert l.result.status == ro["status"]
        sx = check_space(D, K, l, ACC, (dim, cap))
        check_records(l, sx, (dim, cap))
        n, m = sx["n_nodes"], len(sx["child"])
        preds = np.bincount(sx["child"], minlength=n)
        assert preds[0] == 0 and sx["parent"][0] == 0  # the root: an empty predecessor list
        multi = multi or preds.max() > 1
        sizes.append((n, m))
    print("dim", dim, "(states, entries) of the sweep", sizes)
    assert 1 < sizes[0][0] < 10
    assert any(10 <= n < TILE for n, m in sizes)
    assert any(n > TILE and n % TILE and m > TILE and m % TILE for n, m in sizes)
    assert dim == 2 or any(m > TILE * TILE and m % TILE for n, m in sizes)
    assert multi


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_records_split_by_the_blocked_bit_and_changed_primitives(dim):
    D, control = DIMS[dim], ACC
    K, team, l = D.pair(control)
    start, goal = D.endpoints()
    assert l.plan(start, goal) and K.lpa_plan(start, goal)["status"] == 0
    assert check_changed(l, l.space()) == 0           # no updateNodes yet
    act, ids, st = l.traj()
    K.lpa_sub_state_space(1)
    l.sub_state_space(1)
    n_blocked = 0
    for t in (1.0, 2.0, 3.0):
        W = D.world(t, True)
        K.reload(W)
        team.set_worlds([W])
        uo, ud = K.lpa_update_nodes(), l.update_nodes()
        assert ud == uo
        sx = check_space(D, K, l, control, t)
        assert check_changed(l, sx, t) == uo[0] + uo[1]
        nb = check_records(l, sx, t)
        n_blocked += uo[0]
        assert uo[0] == 0 or nb > 0
    assert n_blocked > 0 and nb > 0                   # an updateNodes blocked something: the blocked records are there
    assert l.update_nodes()[:2] == (0, 0)             # the same world again: nothing changes
    rows, action, now = l.changed_primitives()
    assert len(rows) == len(action) == len(now) == 0


def raw_arrays(D, n, m):
    f = {k: np.full(max(n, 1) * (D.W if k == "states" else 1), SENTINEL_D) for k in ("states", "g", "rhs", "h")}
    i = {k: np.full(max(n, 1), SENTINEL_I, dtype=np.int32) for k in ("closed", "opened", "built")}
    r = {k: np.full(max(m, 1), SENTINEL_I, dtype=np.int32) for k in ("entry", "child", "parent", "action", "blocked")}
    return f, i, r


def raw_space(D, l, cap, f, i):
    n = C.c_uint64(99)
    code = D.fn(l.lib, "space")(l.h, cap, f["states"].ctypes.data, f["g"].ctypes.data, f["rhs"].ctypes.data, f["h"].ctypes.data, i["closed"].ctypes.data,
                                i["opened"].ctypes.data, i["built"].ctypes.data, C.byref(n))
    return code, int(n.value)


def raw_records(D, l, which, cap, r):
    n = C.c_uint64(99)
    code = D.fn(l.lib, "records")(l.h, which, cap, r["entry"].ctypes.data, r["child"].ctypes.data, r["parent"].ctypes.data, r["action"].ctypes.data,
                                  r["blocked"].ctypes.data, C.byref(n))
    return code, int(n.value)


def untouched(*dicts):
    return all(np.all(v == (SENTINEL_D if v.dtype == np.float64 else SENTINEL_I)) for d in dicts for v in d.values())


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_empty_spaces_and_small_caps(dim):
    D = DIMS[dim]
    K, team, l = D.pair(ACC)
    start, goal = D.endpoints()
    f, i, r = raw_arrays(D, 64, 64)
    rows = np.full(64 * D.W, SENTINEL_D)

    def nothing(where):
        assert raw_space(D, l, 64, f, i) == (_capi.OK, 0), where
        for which in (0, 1, 2):
            assert raw_records(D, l, which, 64, r) == (_capi.OK, 0), where
        n = C.c_uint64(99)
        assert D.fn(l.lib, "changed")(l.h, 64, rows.ctypes.data, r["action"].ctypes.data, r["blocked"].ctypes.data, C.byref(n)) == _capi.OK and n.value == 0, where
        assert untouched(f, i, r) and np.all(rows == SENTINEL_D), where
        assert l.space()["n_nodes"] == 0 and not l.space()["initialized"], where

    nothing("before any plan")
    at_goal = goal.copy()
    at_goal[0] -= 0.25
    assert l.plan(at_goal, goal) and l.result.n_expanded == 0 and not l.initialized()
    nothing("a start already at the goal")
    assert not l.plan(start, goal, max_expand=30) and l.result.status == _capi.PLAN_MAX_EXPAND
    sx = l.space()
    n, m = sx["n_nodes"], len(sx["child"])
    assert n > 64 and m > 64
    f, i, r = raw_arrays(D, n, m)
    code, cnt = raw_space(D, l, n - 1, f, i)                  # cap one below the count
    assert code == _capi.ERR_CAPACITY and cnt == n and untouched(f, i)
    for which in (0, 1, 2):                                   # cap = 0: a pure count query
        code, cnt = raw_records(D, l, which, 0, r)
        assert code == _capi.OK and cnt == (m, int((sx["blocked"] == 0).sum()), int((sx["blocked"] != 0).sum()))[which] and untouched(r)
    code, cnt = raw_records(D, l, 0, 5, r)                    # at most cap rows are written
    assert code == _capi.OK and cnt == m
    for k in ("child", "parent", "action", "blocked"):
        assert np.array_equal(r[k][:5], sx[k][:5]) and np.all(r[k][5:] == SENTINEL_I), k
    assert np.array_equal(r["entry"][:5], np.arange(5)) and np.all(r["entry"][5:] == SENTINEL_I)
    code, cnt = raw_space(D, l, n, f, i)                      # and the exact cap serves everything
    assert code == _capi.OK and cnt == n and np.array_equal(f["states"].reshape(n, D.W), sx["states"]) and np.array_equal(i["built"], sx["built"])
    g_only = np.full(n, SENTINEL_D)                           # NULL outputs are skipped
    cnt = C.c_uint64()
    assert D.fn(l.lib, "space")(l.h, n, None, g_only.ctypes.data, None, None, None, None, None, C.byref(cnt)) == _capi.OK
    assert np.array_equal(g_only, sx["g"])
    assert all(x >= 0.0 for x in l.export_ms())
    l.reset()
    f, i, r = raw_arrays(D, 64, 64)
    nothing("after reset()")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_many_handles_a_fleet_with_an_empty_a_fresh_and_a_repaired_member(dim):
    D, control = DIMS[dim], ACC
    W0 = D.world(0.0, True)
    team = D.team(control, [W0])
    fleet = team.lpa_fleet([0, 0, 0])
    fleet.set_capacity(1 << 16, 1 << 20, 1 << 20)
    start, goal = D.endpoints()
    goal2 = goal.copy()
    goal2[1] -= 3.0
    S = np.stack([start, start, start]); G = np.stack([goal, goal2, goal])
    res = fleet.plan(S, G, active=[False, False, True])
    assert res[2].status == _capi.PLAN_OK
    act, ids, st = fleet.member(2).traj()
    fleet.sub_state_space([-1, -1, 1])
    team.set_worlds([D.world(1.0, True)])
    upd = fleet.update_nodes()
    assert upd[0][:2] == (0, 0) and upd[2][0] + upd[2][1] > 0
    S[1, D.W - 1] = 1.0
    S[2] = st[1]
    S[2, D.W - 1] = 1.0
    res = fleet.plan(S, G, active=[False, True, True])        # member 1 plans afresh, member 2 repairs, member 0 never planned
    assert res[1].status == res[2].status == _capi.PLAN_OK
    stats = fleet.stats()
    assert stats[0] == 1 and stats[2] == 1, stats
    own = [fleet.member(k).space() for k in range(3)]
    assert own[0]["n_nodes"] == 0 and not own[0]["initialized"] and own[1]["n_nodes"] > TILE and own[2]["n_nodes"] > TILE
    for k in range(3):
        same(own[k], fleet.member(k).state_space(), None, ("member against its host-decoded dump", k))
    for order in ([0, 1, 2], [2, 1, 0]):
        many = fleet.spaces(order)
        for pos, k in enumerate(order):
            same(many[pos], own[k], None, ("spaces() against the member's own space()", order, k))
        counts = [own[k]["n_nodes"] for k in order]
        entries = [len(own[k]["child"]) for k in order]
        assert fleet.last_offsets.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist(), order
        assert fleet.last_entry_offsets.tolist() == np.concatenate([[0], np.cumsum(entries)]).tolist(), order
    # the filtered records of all members in one call: each member's are its own, offsets the prefix of the counts
    hs = (C.c_void_p * 3)(*[fleet.member(k).h.value for k in range(3)])
    for which in (1, 2):
        per = [fleet.member(k).records(which) for k in range(3)]
        tot = sum(len(p["entry"]) for p in per)
        off = np.zeros(4, dtype=np.uint64)
        arr = {k: np.full(max(tot, 1), SENTINEL_I, dtype=np.int32) for k in ("entry", "child", "parent", "action", "blocked")}
        assert D.fn(team.lib, "records_many")(3, hs, which, tot, off.ctypes.data, arr["entry"].ctypes.data, arr["child"].ctypes.data, arr["parent"].ctypes.data,
                                              arr["action"].ctypes.data, arr["blocked"].ctypes.data) == _capi.OK
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(p["entry"]) for p in per])]).tolist(), which
        for k in ("entry", "child", "parent", "action", "blocked"):
            assert np.array_equal(arr[k][:tot], np.concatenate([p[k] for p in per])), (which, k)
    # a planner of another team in the array: refused before any launch
    other = D.team(control, [W0])
    lo = other.lpa()
    assert lo.plan(start, goal, max_expand=5) is False
    mixed = (C.c_void_p * 2)(fleet.member(1).h.value, lo.h.value)
    off = np.zeros(3, dtype=np.uint64)
    g = np.full(8, SENTINEL_D)
    assert D.fn(team.lib, "space_many")(2, mixed, 1 << 20, off.ctypes.data, None, g.ctypes.data, None, None, None, None, None) == _capi.ERR_ARG
    assert b"handle 1 is bound to another" in team.lib.mplx_plpa_export_last_error() and np.all(g == SENTINEL_D)
