"""Scenes of the VoxelGrid sweep (tests/test_grid_geometry.py): named grid geometries, a seeded point generator that
aims at the cell faces, and a seeded operation-sequence generator that covers every form of `allocate` and of
`addCloud(pts, ns)`.  Everything here is plain data: the same sequence is run on the oracle (orc.Grid), on the compiled
reference (RefGrid, where oracle/_ref is built) and on the device grid, and compared after every operation."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RefGrid:
    """The reference's own VoxelGrid, compiled from /root/reference/.../voxel_grid.cpp by `make -C oracle ref`
    (oracle/_ref/libvoxelgrid_ref.so; dependency stand-ins under oracle/ref_stubs)."""
    PATH = os.path.join(ROOT, "oracle", "_ref", "libvoxelgrid_ref.so")

    def __init__(self, origin, dim, res):
        L = C.CDLL(self.PATH)
        D3 = C.c_double * 3
        L.ref_grid_create.restype = C.c_void_p
        L.ref_grid_create.argtypes = [D3, D3, C.c_float]
        for f in ("ref_grid_destroy", "ref_grid_clear", "ref_grid_decay"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.ref_grid_allocate.argtypes = [C.c_void_p, D3, D3]
        L.ref_grid_add_cloud.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.ref_grid_add_cloud_ns.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        for f in ("ref_grid_fill_column", "ref_grid_clear_column"):
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ref_grid_fill_cell.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ref_grid_get_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_void_p]
        L.ref_grid_get_map.restype = C.c_uint64
        L.ref_grid_get_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.ref_grid_get_cloud.restype = C.c_uint64
        self.L, self.D3 = L, D3
        self.h = L.ref_grid_create(D3(*origin), D3(*dim), res)

    def __del__(self):
        try:
            if self.h:
                self.L.ref_grid_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def info(self):
        dim = (C.c_int32 * 3)(); ori = (C.c_double * 3)(); res = C.c_float()
        self.L.ref_grid_get_map(self.h, 0, dim, ori, C.byref(res), None)
        return tuple(dim), tuple(ori), res.value

    def allocate(self, dim, ori):
        return bool(self.L.ref_grid_allocate(self.h, self.D3(*dim), self.D3(*ori)))

    def clear(self, nx=None, ny=None):
        self.L.ref_grid_clear(self.h) if nx is None else self.L.ref_grid_clear_column(self.h, nx, ny)

    def fill(self, nx, ny, nz=None):
        self.L.ref_grid_fill_column(self.h, nx, ny) if nz is None else self.L.ref_grid_fill_cell(self.h, nx, ny, nz)

    def add_cloud(self, pts, ns=None):
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        if ns is None:
            self.L.ref_grid_add_cloud(self.h, p.shape[0], p.ctypes.data)
            return None
        o = np.ascontiguousarray(ns, dtype=np.int32).reshape(-1, 3)
        out = np.empty((max(p.shape[0] * o.shape[0], 1), 3), dtype=np.int32)
        n = self.L.ref_grid_add_cloud_ns(self.h, p.shape[0], p.ctypes.data, o.shape[0], o.ctypes.data, out.ctypes.data, out.shape[0])
        return out[:n]

    def decay(self):
        self.L.ref_grid_decay(self.h)

    def get_map(self, inflated=False):
        dim, _, _ = self.info()
        data = np.empty(dim[0] * dim[1] * dim[2], dtype=np.int8)
        d = (C.c_int32 * 3)(); o = (C.c_double * 3)(); r = C.c_float()
        self.L.ref_grid_get_map(self.h, 1 if inflated else 0, d, o, C.byref(r), data.ctypes.data)
        return data

    def get_cloud(self):
        n = int(self.L.ref_grid_get_cloud(self.h, None, 0))
        out = np.empty((max(n, 1), 3), dtype=np.float64)
        self.L.ref_grid_get_cloud(self.h, out.ctypes.data, n)
        return out[:n]


# ---------------------------------------------------------------------------------------------------------------- geometries
def f32(x):
    return float(np.float32(x))


def cells_of(dim_d, ori_d, res):
    """VoxelGrid::allocate's cell counts and integer origin (voxel_grid.cpp:130-132): truncating division by the FLOAT
    resolution, and the flat rule"""
    r = f32(res)
    nd = [int(float(d) / r) for d in dim_d]
    no = [int(float(o) / r) for o in ori_d]
    if nd[2] == 0 and no[2] == 0:
        nd[2] = 1
    return tuple(nd), tuple(no)


def _scene(origin, res, cells=None, size=None, large=False, what=""):
    # a metric size half a cell past the intended count: float32(0.1) > 0.1, so 3.7 m / 0.1f holds 36 cells, not 37
    if size is None:
        size = tuple((c + 0.5) * f32(res) for c in cells)
    return {"origin": tuple(float(o) for o in origin), "res": res, "size": tuple(float(s) for s in size), "cells": tuple(cells),
            "large": large, "what": what}


SCENES = {
    "neg_unaligned": _scene((-3.07, -2.01, -0.33), 0.1, (37, 29, 11), what="negative origin that is no multiple of the resolution"),
    "pos_far": _scene((48.37, 22.63, 1.07), 0.05, (45, 33, 13), what="far positive origin: large quotients, integer origin ~1000"),
    "r025_exact": _scene((-4.0, -4.0, 0.0), 0.25, (32, 24, 10), size=(8.0, 6.0, 2.5), what="binary-exact resolution: points on cell faces are exact"),
    "r03": _scene((1.0, -2.5, 0.2), 0.3, (23, 17, 7), what="resolution 0.3"),
    "third": _scene((-1.0, 0.5, -0.7), 1.0 / 3.0, (19, 21, 5), what="resolution 1/3"),
    "flat": _scene((-2.0, -1.5, 0.0), 0.1, (40, 30, 1), size=(40.5 * f32(0.1), 30.5 * f32(0.1), 0.0), what="z size 0 at z origin 0: the flat rule gives one layer"),
    "line_x": _scene((0.3, 0.3, 0.3), 0.1, (57, 1, 1), what="1-cell axes"),
    "one_cell": _scene((0.5, -0.5, 0.25), 0.2, (1, 1, 1), what="a single cell"),
    "scan_1023": _scene((-1.65, -1.55, 0.0), 0.1, (33, 31, 3), what="1023 columns: one scan chunk less one"),
    "scan_1024": _scene((-1.6, -1.6, 0.0), 0.1, (32, 32, 3), what="1024 columns: exactly one scan chunk"),
    "scan_1025": _scene((-2.05, -1.25, 0.0), 0.1, (41, 25, 3), what="1025 columns: a second scan chunk of one column"),
    "cells_over_stride": _scene((-6.4, -6.4, -1.0), 0.1, (128, 128, 80), large=True, what="1 310 720 cells: the 4096 x 256 grid-stride loops iterate"),
    "cols_over_stride": _scene((-27.5, -24.0, 0.0), 0.05, (1100, 960, 2), large=True, what="1 056 000 columns: the column loops iterate, 1032 scan chunks"),
}
# a refusal, not a geometry: z size 0 off z origin 0 gives nd[2] = 0, which the device refuses ("empty grid")
FLAT_OFF = {"origin": (-2.0, -1.5, 0.5), "res": 0.1, "size": (40.5 * f32(0.1), 30.5 * f32(0.1), 0.0)}

SEEDS = {name: 1000 + i for i, name in enumerate(SCENES)}

NS_18 = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (0, 1)]  # the neighbourhood of tests/test_voxel_grid.py
NS_RING3 = [(x, y, z) for x in (-3, 0, 3) for y in (-3, 0, 3) for z in (-3, 0, 3) if (x, y, z) != (0, 0, 0)]  # several cells, no centre
NS_DUP = [(1, 0, 0), (0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 0), (-2, 1, 0), (0, -1, 0)]  # duplicated offsets
NS_SETS = {"empty": [], "centre": [(0, 0, 0)], "18": NS_18, "ring3": NS_RING3, "dup": NS_DUP}


# ---------------------------------------------------------------------------------------------------------------- points
LAUNCH_THREADS = 4096 * 256  # grid_decay / grid_get_map / grid_realloc / cloud_count / cloud_write: a grid-stride loop beyond this


def make_points(rng, origin, cells, res, n_inside):
    """A cloud on the grid (origin, cells, float32 res), all classes shuffled together: uniform inside; within one cell of each
    of the six faces, on both sides (just below the origin truncates INTO cell 0); exactly on cell faces (origin + k * res in
    double, k = 0, dim and in between); repeated cells; a block in one cell; far outside (+-1e6, +-1e300, +-inf); on the two
    large scenes also the rows of cells around each multiple of the launch size."""
    o, nd, r = np.array(origin, dtype=np.float64), np.array(cells, dtype=np.float64), f32(res)
    out = []
    inside = o + rng.uniform(0.0, 1.0, (n_inside, 3)) * nd * r
    out.append(inside)
    # both sides of the six faces
    for axis in range(3):
        for face in (0.0, nd[axis]):
            p = o + rng.uniform(0.0, 1.0, (8, 3)) * nd * r
            p[:, axis] = o[axis] + (face + rng.uniform(-1.0, 1.0, 8)) * r
            p[0, axis] = o[axis] + (face - 1e-9) * r  # a hair on either side
            p[1, axis] = o[axis] + (face + 1e-9) * r
            out.append(p)
    # exactly on cell faces, in one, two and three coordinates
    k = np.stack([rng.integers(0, int(nd[a]) + 1, 18) for a in range(3)], axis=1).astype(np.float64)
    k[0] = 0.0
    k[1] = nd
    k[2] = (0.0, nd[1], 0.0)
    on = o + k * r
    free = o + rng.uniform(0.0, 1.0, (18, 3)) * nd * r
    mask = rng.integers(0, 2, (18, 3)).astype(bool)
    mask[:3] = True
    out.append(np.where(mask, on, free))
    # repeated cells: copies of earlier points, and other points of the same cells
    rep = inside[rng.integers(0, n_inside, max(n_inside // 4, 4))]
    out.append(rep)
    cell = np.floor((rep - o) / r)
    out.append(o + (cell + rng.uniform(0.2, 0.8, cell.shape)) * r)
    # a block of points all in one cell
    c1 = np.array([rng.integers(0, int(nd[a])) for a in range(3)], dtype=np.float64)
    out.append(o + (c1 + rng.uniform(0.2, 0.8, (20, 3))) * r)
    # far outside, one coordinate at a time and all three
    far = []
    for v in (1e6, -1e6, 1e300, -1e300, np.inf, -np.inf):
        for axis in range(3):
            p = o + rng.uniform(0.0, 1.0, 3) * nd * r
            p[axis] = v
            far.append(p)
        far.append(np.array([v, v, v]))
    out.append(np.array(far))
    # where the cells, or the columns, outnumber the threads of the 4096 x 256 launches: every cell of the rows on either side
    # of each multiple of that count (x-fastest index), so that a loop that strides a block too far skips occupied cells
    for count, layers in ((int(nd[0] * nd[1] * nd[2]), 1), (int(nd[0] * nd[1]), int(nd[2]))):
        for edge in range(LAUNCH_THREADS, count, LAUNCH_THREADS):
            idx = np.arange(edge - 128, min(edge + 640, count))
            cell = np.stack([idx % int(nd[0]), (idx // int(nd[0])) % int(nd[1]), idx // int(nd[0] * nd[1])], axis=1).astype(np.float64)
            for z in range(layers if layers > 1 else 1):
                c = cell.copy()
                if layers > 1:
                    c[:, 2] = z
                out.append(o + (c + 0.5) * r)
    pts = np.concatenate(out)
    rng.shuffle(pts)
    return np.ascontiguousarray(pts)


# ---------------------------------------------------------------------------------------------------------------- operations
def _allocate_args(form, rng, cur, home):
    """(size, origin) of one `allocate` form, from the current geometry `cur` = (origin_d, cells) and the scene's first one."""
    (o, nd), r = cur, home["r"]
    o, nd = np.array(o, dtype=np.float64), np.array(nd)
    size = lambda c: tuple(float((ci + 0.5) * r) for ci in c)  # noqa: E731
    if form == "same":
        return size(nd), tuple(o)
    if form == "grow":
        a, b = rng.integers(1, 4, 3), rng.integers(1, 4, 3)
        return size(nd + a + b), tuple(o - a * r)
    if form == "shrink":  # as far as an axis has cells to give
        a = np.minimum(rng.integers(1, 4, 3), (nd - 1) // 2)
        b = np.minimum(rng.integers(1, 4, 3), (nd - 1) // 2)
        return size(nd - a - b), tuple(o + a * r)
    if form == "shift_up":
        return size(nd), tuple(o + rng.integers(1, 4, 3) * r)
    if form == "shift_down":
        return size(nd), tuple(o - rng.integers(1, 4, 3) * r)
    if form == "disjoint":  # past the far x face: no cell carries over
        return size(nd), (float(o[0] + (nd[0] + 2) * r), float(o[1]), float(o[2]))
    if form == "origin_only":  # one axis, the size untouched
        axis = int(rng.integers(0, 2))
        d = np.zeros(3)
        d[axis] = 2 * r
        return size(nd), tuple(o + d)
    if form == "size_only":
        return size(nd + np.array([2, 1, 0 if nd[2] == 1 else 2])), tuple(o)
    if form == "flat":  # 3-D to flat: z size 0 at z origin 0 (one layer, the integer layer 0 of the old grid if it had one)
        s = size(nd)
        return (s[0], s[1], 0.0), (float(o[0]), float(o[1]), 0.0)
    if form == "home":  # ... and back
        return home["size"], home["origin"]
    if form == "thick":  # a flat scene's way to 3-D (and "home" brings it back to one layer)
        s = size(nd)
        return (s[0], s[1], 4.5 * r), (float(o[0]), float(o[1]), float(-2 * r))
    raise KeyError(form)


def make_sequence(name):
    """The scene's operation sequence, as plain data: a list of tuples
        ("add", pts) | ("add_ns", pts, ns, ns_name) | ("decay", times) | ("fill", nx, ny) | ("fill", nx, ny, nz) | ("clear", nx, ny)
        | ("clear",) | ("allocate", size, origin, form, (origin_d, cells) expected afterwards)
    `clear(nx, ny)` only gets in-range columns (the reference's has no bounds test).  Every sequence has an addCloud(pts, ns)
    after an allocate and after a decay."""
    sc = SCENES[name]
    rng = np.random.default_rng(SEEDS[name])
    r = f32(sc["res"])
    home = {"r": r, "size": sc["size"], "origin": sc["origin"]}
    cur = [sc["origin"], cells_of(sc["size"], sc["origin"], sc["res"])[0], cells_of(sc["size"], sc["origin"], sc["res"])[1]]
    assert cur[1] == sc["cells"], (name, cur[1])
    n_inside = 2500 if sc["large"] else max(8, min(300, int(np.prod(sc["cells"])) // 6))
    ops = []

    def pts():
        return make_points(rng, cur[0], cur[1], sc["res"], n_inside)

    def add():
        ops.append(("add", pts()))

    def add_ns(which, p=None):
        ops.append(("add_ns", pts() if p is None else p, NS_SETS[which], which))

    def decay(times):
        ops.append(("decay", times))

    def col(in_range):
        nd = cur[1]
        if in_range:
            return int(rng.integers(0, nd[0])), int(rng.integers(0, nd[1]))
        return [(-1, 0), (0, -1), (nd[0], 0), (0, nd[1]), (nd[0] + 7, nd[1] + 7)][int(rng.integers(0, 5))]

    def fill2(in_range=True):
        ops.append(("fill",) + col(in_range))

    def fill3(in_range=True):
        nd = cur[1]
        c = col(True) + (int(rng.integers(0, nd[2])),) if in_range else [col(False) + (0,), col(True) + (-1,), col(True) + (nd[2],)][int(rng.integers(0, 3))]
        ops.append(("fill",) + tuple(c))

    def clear2():
        ops.append(("clear",) + col(True))

    def allocate(form):
        size, origin = _allocate_args(form, rng, (cur[0], cur[1]), home)
        nd, no = cells_of(size, origin, sc["res"])
        if nd != cur[1] or no != cur[2]:  # allocate returns false, and keeps origin_d, when the integers do not change
            cur[0], cur[1], cur[2] = tuple(origin), nd, no
        ops.append(("allocate", size, origin, form, (cur[0], cur[1])))  # ... with the geometry expected afterwards

    flat_scene = sc["cells"][2] == 1 and sc["size"][2] == 0.0
    if sc["large"]:  # 13 operations, sparse clouds
        # (the second cloud again right after the decay, on the same geometry: a cell the decay skipped stays at 100 and keeps quiet)
        add(); add_ns("18"); decay(1); add_ns("ring3", ops[1][1]); allocate("grow"); add_ns("18"); ops.append(("clear",)); fill2(); fill2(False); fill3(); clear2()
        allocate("disjoint"); add_ns("dup")  # (the filled cells do not carry over)
        return ops
    add(); add_ns("18"); decay(1); add_ns("18", ops[1][1])  # the same cloud again: cells that decayed to 99 flip once more
    body = [lambda f=f: allocate(f) for f in ("same", "grow", "shrink", "shift_up", "shift_down", "origin_only", "size_only")]
    body += [lambda w=w: add_ns(w) for w in ("empty", "centre", "18", "ring3", "dup")]
    body += [add, add, lambda: decay(1), lambda: decay(2), lambda: decay(3), fill2, fill2, lambda: fill2(False), fill3, fill3,
             lambda: fill3(False), clear2, clear2, lambda: ops.append(("clear",))]
    for i in rng.permutation(len(body)):
        body[int(i)]()
    # the forms that lose (nearly) everything come last, each followed by a cloud
    allocate("thick" if flat_scene else "flat"); add_ns("18"); allocate("home"); add_ns("ring3"); decay(1)
    allocate("disjoint"); add_ns("dup"); allocate("grow"); add_ns("18"); decay(2); add_ns("centre", ops[-2][1])
    return ops


_SEQ_CACHE = {}


def sequence(name):
    """make_sequence(name), built once per process and shared (the arrays are read-only)"""
    if name not in _SEQ_CACHE:
        ops = make_sequence(name)
        for op in ops:
            if op[0] in ("add", "add_ns"):
                op[1].setflags(write=False)
        _SEQ_CACHE[name] = ops
    return _SEQ_CACHE[name]


def apply(G, op):
    """One operation on any of the three implementations; returns new_obs (add_ns), the allocate flag, or None."""
    add = G.addCloud if hasattr(G, "addCloud") else G.add_cloud
    if op[0] == "add":
        return add(op[1])
    if op[0] == "add_ns":
        return add(op[1], np.array(op[2], dtype=np.int32).reshape(-1, 3))
    if op[0] == "decay":
        for _ in range(op[1]):
            G.decay()
        return None
    if op[0] == "fill":
        return G.fill(*op[1:])
    if op[0] == "clear":
        return G.clear(*op[1:])
    if op[0] == "allocate":
        return G.allocate(op[1], op[2])
    raise KeyError(op[0])


def state(G):
    """(info, map, inflated map, cloud) of any of the three implementations"""
    if hasattr(G, "getMap"):
        return G.info(), G.getMap()["data"], G.getInflatedMap()["data"], G.getCloud()
    return G.info(), G.get_map(), G.get_map(True), G.get_cloud()


def assert_same_state(a, b, where):
    assert a[0] == b[0], (where, "info", a[0], b[0])
    assert np.array_equal(a[1], b[1]), (where, "map", int((a[1] != b[1]).sum()))
    assert np.array_equal(a[2], b[2]), (where, "inflated map", int((a[2] != b[2]).sum()))
    # f64 bit patterns, and the order
    assert a[3].shape == b[3].shape and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), (where, "cloud", a[3].shape, b[3].shape)


def assert_same_result(ra, rb, where):
    if isinstance(ra, np.ndarray) or isinstance(rb, np.ndarray):
        assert ra.shape == rb.shape and np.array_equal(ra, rb), (where, "new_obs", ra.shape, rb.shape)
    else:
        assert ra == rb, (where, "return", ra, rb)


def run_lockstep(name, grids, after_op=None):
    """The scene's sequence on several implementations at once: every result and the whole state compared with grids[0]
    after every operation."""
    sc = SCENES[name]
    G = [make(sc["origin"], sc["size"], sc["res"]) for make in grids]
    ref = state(G[0])
    for g in G[1:]:
        assert_same_state(ref, state(g), (name, "constructor"))
    for i, op in enumerate(sequence(name)):
        where = (name, i, op[0], op[3] if op[0] in ("add_ns", "allocate") else op[1:] if op[0] in ("fill", "clear", "decay") else "")
        res = [apply(g, op) for g in G]
        ref = state(G[0])
        for r, g in zip(res[1:], G[1:]):
            assert_same_result(res[0], r, where)
            assert_same_state(ref, state(g), where)
        if after_op is not None:
            after_op(i, op, res[0], ref)
    return G
