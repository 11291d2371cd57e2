"""The device-side state-space exports of the moving-obstacle LPA* planners (mplx_plpa_export_* / mplx_plpa3_export_*), shared by
PolyLpa / PolyLpaFleet (poly_map.py, rows of 9 doubles) and PolyLpa3D / PolyLpaFleet3D (poly_map3d.py, rows of 13): the passes run
over the handles' pools on the device and only the result arrays cross the bus."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import MplxError

WHICH_ALL, WHICH_VALID, WHICH_BLOCKED = 0, 1, 2


def _fn(lib, prefix, name):
    return getattr(lib, f"mplx_{prefix}_export_{name}")


def _check(lib, code):
    if code != _capi.OK:
        raise MplxError(f"mplx error {code}: {lib.mplx_plpa_export_last_error().decode()}")


def _space_dict(n, states, g, rhs, h, closed, opened, built, rec, initialized):
    return dict(n_nodes=n, states=states, g=g, rhs=rhs, h=h, closed=closed, opened=opened, built=built,
                child=rec["child"], parent=rec["parent"], action=rec["action"], blocked=rec["blocked"], initialized=initialized)


def counts(lib, prefix, h):
    """(states, entries) of the handle's space (host bookkeeping: no device work)"""
    nn, ne = C.c_uint64(), C.c_uint64()
    if getattr(lib, f"mplx_{prefix}_counts")(h, C.byref(nn), C.byref(ne)) != _capi.OK:
        raise MplxError(f"mplx_{prefix}_counts failed")
    return int(nn.value), int(ne.value)


def records(lib, prefix, h, which=WHICH_ALL):
    """the predecessor entries in creation order, filtered: dict(entry, child, parent, action, blocked)"""
    cap = counts(lib, prefix, h)[1]  # (the filter keeps at most every entry: one call)
    n = C.c_uint64()
    a = {k: np.zeros(max(cap, 1), dtype=np.int32) for k in ("entry", "child", "parent", "action", "blocked")}
    _check(lib, _fn(lib, prefix, "records")(h, int(which), cap, a["entry"].ctypes.data, a["child"].ctypes.data, a["parent"].ctypes.data,
                                            a["action"].ctypes.data, a["blocked"].ctypes.data, C.byref(n)))
    m = int(n.value)
    return {k: v[:m] for k, v in a.items()}


def space(lib, prefix, W, h, initialized):
    """the dict of state_space(), key for key, from the export"""
    n = counts(lib, prefix, h)[0]
    states = np.zeros((max(n, 1), W)); g = np.zeros(max(n, 1)); rhs = np.zeros(max(n, 1)); hh = np.zeros(max(n, 1))
    closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy(); built = closed.copy()
    cnt = C.c_uint64()
    _check(lib, _fn(lib, prefix, "space")(h, max(n, 1), states.ctypes.data, g.ctypes.data, rhs.ctypes.data, hh.ctypes.data, closed.ctypes.data,
                                          opened.ctypes.data, built.ctypes.data, C.byref(cnt)))
    assert int(cnt.value) == n
    rec = records(lib, prefix, h, WHICH_ALL)
    return _space_dict(n, states[:n], g[:n], rhs[:n], hh[:n], closed[:n], opened[:n], built[:n], rec, initialized)


def changed_primitives(lib, prefix, W, h):
    """of the last updateNodes, in the order of changed(): (parent states n x W, actions, now-blocked bits)"""
    n = C.c_uint64()
    _check(lib, _fn(lib, prefix, "changed")(h, 0, None, None, None, C.byref(n)))
    m = int(n.value)
    rows = np.zeros((max(m, 1), W)); action = np.zeros(max(m, 1), dtype=np.int32); now_blocked = action.copy()
    if m:
        _check(lib, _fn(lib, prefix, "changed")(h, m, rows.ctypes.data, action.ctypes.data, now_blocked.ctypes.data, C.byref(n)))
    return rows[:m], action[:m], now_blocked[:m]


def export_ms(lib, prefix, h):
    """kernel ms of the handle's last space / records / changed export"""
    ms = (C.c_float * 3)()
    _check(lib, _fn(lib, prefix, "ms")(h, ms))
    return [float(x) for x in ms]


def spaces(lib, prefix, W, handles, initialized):
    """the space() dict of every handle (all bound to one planner object), one launch per pass"""
    k = len(handles)
    arr = (C.c_void_p * k)(*[x.value if isinstance(x, C.c_void_p) else x for x in handles])
    off = np.zeros(k + 1, dtype=np.uint64)
    cnt = [counts(lib, prefix, x) for x in arr]
    n, m = sum(c[0] for c in cnt), sum(c[1] for c in cnt)
    states = np.zeros((max(n, 1), W)); g = np.zeros(max(n, 1)); rhs = np.zeros(max(n, 1)); hh = np.zeros(max(n, 1))
    closed = np.zeros(max(n, 1), dtype=np.int32); opened = closed.copy(); built = closed.copy()
    _check(lib, _fn(lib, prefix, "space_many")(k, arr, max(n, 1), off.ctypes.data, states.ctypes.data, g.ctypes.data, rhs.ctypes.data, hh.ctypes.data,
                                               closed.ctypes.data, opened.ctypes.data, built.ctypes.data))
    eoff = np.zeros(k + 1, dtype=np.uint64)
    rec = {key: np.zeros(max(m, 1), dtype=np.int32) for key in ("child", "parent", "action", "blocked")}
    _check(lib, _fn(lib, prefix, "records_many")(k, arr, WHICH_ALL, m, eoff.ctypes.data, None, rec["child"].ctypes.data, rec["parent"].ctypes.data,
                                                 rec["action"].ctypes.data, rec["blocked"].ctypes.data))
    assert int(off[k]) == n and int(eoff[k]) == m
    out = []
    for i in range(k):
        a, b, ea, eb = int(off[i]), int(off[i + 1]), int(eoff[i]), int(eoff[i + 1])
        out.append(_space_dict(b - a, states[a:b], g[a:b], rhs[a:b], hh[a:b], closed[a:b], opened[a:b], built[a:b],
                               {key: v[ea:eb] for key, v in rec.items()}, initialized[i]))
    return out, off, eoff
