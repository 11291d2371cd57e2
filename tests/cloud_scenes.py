"""Seeded point clouds for the point-cloud planner's tests: an "office-shaped" scene that matches
mpl_test_node/launch/ellipsoid_planner_node/test.launch (box origin (6, 12, 0), range (25, 5, 1.5), start (8, 13, 1.3),
goal (28.5, 14, 1.3)) -- outer walls, partition walls with doorways, pillars and desks as points on a 0.05 m lattice,
every coordinate a float32 value, plus a handful of points outside the box -- and the launch file's parameters; and SCENES, the
table of named scenes with their seeded builders that tests/test_cloud_geometry.py sweeps."""
import math

import numpy as np

ORI, DIM = (6.0, 12.0, 0.0), (25.0, 5.0, 1.5)
START, GOAL = (8.0, 13.0, 1.3), (28.5, 14.0, 1.3)
LAUNCH = dict(dt=0.2, v_max=10.0, a_max=10.0, u_max=60.0, num=2, w=10000.0, eps=2.0, tol=(2.0, 2.0, 100.0), r=0.5)
STEP = 0.05


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _span(lo, hi):
    n = int(round((hi - lo) / STEP))
    return lo + STEP * np.arange(n + 1)


def wall_x(x, y0, y1, z0=0.0, z1=1.5):
    """a wall in the plane x = const"""
    yy, zz = np.meshgrid(_span(y0, y1), _span(z0, z1), indexing="ij")
    return np.stack([np.full(yy.size, x), yy.ravel(), zz.ravel()], axis=1)


def wall_y(y, x0, x1, z0=0.0, z1=1.5):
    xx, zz = np.meshgrid(_span(x0, x1), _span(z0, z1), indexing="ij")
    return np.stack([xx.ravel(), np.full(xx.size, y), zz.ravel()], axis=1)


def pillar(cx, cy, rad=0.2, z1=1.5):
    n = max(8, int(2 * np.pi * rad / STEP))
    a = 2 * np.pi * np.arange(n) / n
    zz = _span(0.0, z1)
    return np.array([(cx + rad * np.cos(t), cy + rad * np.sin(t), z) for t in a for z in zz])


def desk(x0, y0, x1, y1, top=0.75):
    xx, yy = np.meshgrid(_span(x0, x1), _span(y0, y1), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, top)], axis=1)


def office(seed=0):
    """(N, 3) float64 points, every one a float32 value.  The start and goal are free and a path exists: the partitions
    leave 2 m doorways (the robot's ellipsoid is 1 m across) and nothing stands above desk height in the corridor."""
    rng = np.random.default_rng(seed)
    parts = [wall_y(12.0, 6.0, 31.0), wall_y(17.0, 6.0, 31.0), wall_x(6.0, 12.0, 17.0), wall_x(31.0, 12.0, 17.0),
             wall_x(12.0, 12.0, 14.6), wall_x(18.0, 14.4, 17.0), wall_x(24.0, 12.0, 14.6),
             pillar(15.0, 13.0), pillar(21.0, 16.0), pillar(27.0, 13.0),
             desk(7.0, 15.5, 9.0, 16.5), desk(19.5, 12.3, 21.5, 13.0), desk(25.5, 15.8, 28.0, 16.7)]
    pts = np.concatenate(parts)
    outside = np.array([[10.0, 11.85, 1.3], [16.5, 17.2, 1.2], [22.0, 11.7, 1.6], [29.0, 17.3, 0.4], [5.8, 14.0, 1.3]])
    outside = outside + rng.uniform(-0.05, 0.05, size=outside.shape)
    return _f32(np.concatenate([pts, outside]))


def start_goal(control=3):
    from mpl_ros_amd.ellipsoid import state13
    return state13(START), state13(GOAL)


# ------------------------------------------------------------------------------------------------------------ the scene table
# Named scenes of the point-cloud sweep (tests/test_cloud_geometry.py), after the model of util.GEOMETRIES.  Each entry: the box
# (ori, dim), the robot radius r, dt, the lattice (inputs of +-u[control] per axis in `num` steps, planar or 3-D), the limits, the
# speed of the seeded states, the control kinds it runs with and the name of its builder.  A builder returns (points, states) for one
# control kind; every cloud is generated from the scene's seed, none is stored.
VEL, ACC, JRK, SNP = 1, 3, 7, 15
ALL_KINDS = (VEL, ACC, JRK, SNP)
U_DEFAULT = {VEL: 3.0, ACC: 20.0, JRK: 100.0, SNP: 1000.0}
CELL_MARGIN = 1.0625  # cell edge of the device index / float32(r) (mplx_cloud.h)


def _scene(ori, dim, r, build, controls=ALL_KINDS, dt=0.2, u=None, num=1, use_3d=True, v_max=10.0, a_max=40.0, j_max=-1.0, vel=3.0,
           n_states=48, seed=1, **extra):
    return dict(ori=tuple(ori), dim=tuple(dim), r=r, build=build, controls=tuple(controls), dt=dt, u=dict(U_DEFAULT if u is None else u),
                num=num, use_3d=use_3d, v_max=v_max, a_max=a_max, j_max=j_max, vel=vel, n_states=n_states, seed=seed, **extra)


EQ = dict(controls=(ACC,), u={ACC: 10.0}, use_3d=False, r=0.5, n_states=60, build="equator")
SCENES = {
    # ---- box origins and radii: seeded states, points just inside / outside ellipsoids the planner tests, a scatter of strangers
    "neg_r05": _scene((-17.37, -9.21, -3.13), (10.0, 8.0, 3.0), 0.5, "surface", seed=11),
    "mixed_r0625": _scene((-3.13, 1.07, -1.52), (9.0, 7.0, 3.0), 0.625, "surface", seed=12),
    "far1e3_r03": _scene((1003.37, 998.21, -1001.3), (8.0, 9.0, 3.0), 0.3, "surface", seed=13),
    "farm1e4_r005": _scene((-10002.29, -9997.43, -10001.17), (7.0, 6.0, 2.5), 0.05, "surface", seed=14, vel=2.0, n_states=40),
    "far1e5_r2": _scene((100003.37, 99998.21, 100001.3), (40.0, 36.0, 8.0), 2.0, "surface", seed=15, scatter=500),
    # ---- the float-filter regime: resting states, n = 1, point pairs on the equator of the t = dt ellipsoid
    "eq_origin": _scene((-6.63, -7.21, -1.13), (13.6, 13.6, 2.0), seed=21, **EQ),
    "eq_1e3": _scene((1003.37, 998.21, 1001.3), (13.6, 13.6, 2.0), seed=22, **EQ),
    "eq_m1e4": _scene((-10002.29, -9997.43, -10001.17), (13.6, 13.6, 2.0), seed=23, **EQ),
    "eq_1e5": _scene((100003.37, 99998.21, 100001.3), (13.6, 13.6, 2.0), seed=24, **EQ),
    # ---- points on the faces of the index's cells, at positive and negative cell indices; sample centres in the neighbouring cells
    "cell_faces": _scene((-6.11, -5.87, -4.93), (12.0, 12.0, 10.0), 0.5, "cell_faces", controls=(ACC,), u={ACC: 0.25}, dt=0.4, n_states=64,
                         seed=31),
    # ---- the strict < of the radius filter
    "knife_edge": _scene((-8.13, -6.29, -1.07), (16.0, 12.0, 2.0), 0.625, "knife_edge", controls=(VEL,), u={VEL: 2.0}, dt=0.25, use_3d=False,
                         n_states=8, seed=32),
    # ---- index sizes: tables where most of the 27 cells share a bucket, the scan kernel's slice change, one crowded bucket
    **{f"index_{n}": _scene((-4.37, 2.21, -1.13), (9.0, 8.0, 3.0), 0.5, "index", controls=(ACC,), n_states=24, seed=40 + i, n_pts=n)
       for i, n in enumerate((1, 2, 3, 5, 8))},
    **{f"index_{n}": _scene((-4.37, 2.21, -1.13), (9.0, 8.0, 3.0), 0.5, "index", controls=(JRK,), n_states=40, seed=50 + i, n_pts=n)
       for i, n in enumerate((1023, 1024, 1025, 3001))},
    "index_copies": _scene((-4.37, 2.21, -1.13), (9.0, 8.0, 3.0), 0.5, "copies", controls=(ACC,), n_states=40, seed=60, copies=4096),
    # ---- NaN, +-inf, 1e300 (float32 inf) and 1e30 among the points of a working cloud
    "nonfinite": _scene((-3.13, 1.07, -1.52), (9.0, 7.0, 3.0), 0.5, "nonfinite", controls=(ACC, SNP), seed=70),
    # ---- a far-away room for whole plans: a wall across it with a 2 m doorway, and a sealed closet in one corner
    "door_1e3": _scene((1003.37, -997.79, 1001.3), (12.0, 6.0, 2.0), 0.5, "door", u={VEL: 2.5, ACC: 10.0, JRK: 50.0, SNP: 100.0}, use_3d=False,
                       v_max=3.0, a_max=20.0, j_max=-1.0, vel=2.0, seed=90, n_states=40, closet=(10.5, 1.5, 1.0),
                       pairs=dict(hard=((3.0, 5.2, 1.0), (9.0, 5.2, 1.0)), easy=((5.0, 3.0, 1.0), (9.5, 4.5, 1.0)),
                                  diag=((1.5, 0.8, 1.0), (10.5, 5.0, 1.0)))),
    # ---- sampling edges of one expansion: a single input and 256 of them; max_v dt / r an exact integer; a primitive of 261 ellipsoids
    # (two staging chunks); 256 and 257 (primitive, ellipsoid) pairs in one state; a primitive only the t = dt / 2 box sample rejects
    "nu_1": _scene((-17.37, -9.21, -3.13), (10.0, 8.0, 3.0), 0.5, "surface", controls=(ACC,), seed=81, U=((20.0, -10.0, 5.0),), n_states=100,
                   near_every=3),
    "nu_256": _scene((-17.37, -9.21, -3.13), (10.0, 8.0, 3.0), 0.5, "surface", controls=(ACC,), seed=82, n_states=24,
                     U=tuple((4.0 * i - 30.0, 4.0 * j - 30.0, 2.0 * ((i + j) % 3 - 1)) for i in range(16) for j in range(16))),
    "ceil_edge": _scene((-3.13, 1.07, -1.52), (9.0, 7.0, 3.0), 0.5, "ceil_edge", controls=(VEL,), dt=0.25, seed=83, n_states=6,
                        U=((4.0, 0.0, 0.0), (0.0, 4.0, 0.0), (2.0, 0.0, 0.0), (-4.0, 0.0, 0.0), (0.0, -3.0, 0.0))),
    "long_261": _scene((1003.37, 998.21, -1001.32), (16.0, 4.0, 2.0), 0.05, "long", controls=(VEL,), dt=1.0, v_max=20.0, seed=84, n_states=6,
                       U=((13.0, 0.0, 0.0), (0.0, 1.0, 0.0))),
    "pairs_256_257": _scene((-10002.29, -9997.43, -10001.17), (16.0, 8.0, 2.0), 0.05, "pair_totals", controls=(VEL,), dt=1.0, seed=85,
                            n_states=8, U=((7.49, 0.0, 0.0), (0.0, 5.19, 0.0), (0.0, -5.24, 0.0))),
    "mid_box": _scene((-3.13, 1.07, -1.52), (9.0, 7.0, 3.0), 0.5, "mid_box", controls=(ACC,), a_max=50.0, seed=86, n_states=6,
                      U=((-40.0, 0.0, 0.0), (40.0, 0.0, 0.0), (0.0, -40.0, 0.0), (0.0, 40.0, 0.0), (0.0, 0.0, 0.0))),
}
INDEX_SIZES = (1, 2, 3, 5, 8, 1023, 1024, 1025, 3001)


def lattice(sc, control):
    from mpl_ros_amd.ellipsoid import control_lattice
    if "U" in sc:
        return np.array(sc["U"], dtype=np.float64)
    u = sc["u"][control]
    return control_lattice(u, sc["num"], sc["use_3d"], u / 2)


def checker(sc, control, pts, U=None, brute=True, cloud=None, cls=None):
    """the CPU checker of scene sc on cloud `pts` (brute mode unless told otherwise)"""
    from tests import cloud_checker as K
    cl = cloud if cloud is not None else K.Cloud(pts, sc["r"], sc["ori"], sc["dim"], brute=brute)
    return (cls or K.Checker)(cl, control, lattice(sc, control) if U is None else U, sc["dt"], v_max=sc["v_max"], a_max=sc["a_max"], j_max=sc["j_max"])


def random_states(rng, n, lo, hi, control, vel=3.0, acc=3.0, jrk=10.0):
    st = np.zeros((n, 13))
    st[:, 0:3] = rng.uniform(lo, hi, size=(n, 3))
    if control & 2:
        st[:, 3:6] = rng.uniform(-vel, vel, size=(n, 3))
    if control & 4:
        st[:, 6:9] = rng.uniform(-acc, acc, size=(n, 3))
    if control & 8:
        st[:, 9:12] = rng.uniform(-jrk, jrk, size=(n, 3))
    st[:, 12] = rng.uniform(0, 5, size=n)
    return st


def primitive(ck, s13, i):
    import ctypes as C
    from oracle import orc
    from tests import cloud_checker as K
    pr = orc.Primitive()
    w = K.state_wp(s13, ck.control)
    orc.lib().orc_primitive_build(C.byref(w), (C.c_double * 3)(*ck.U[i]), ck.dt, C.byref(pr))
    return pr


def max_vel(pr):
    import ctypes as C
    from oracle import orc
    return max([0.0] + [orc.lib().orc_primitive_max_vel(C.byref(pr), k) for k in range(3)])


def n_of(pr, dt, r):
    """n of E6: the primitive's ellipsoids are j = 0..n"""
    return int(math.ceil(max_vel(pr) * dt / r))


def sample(pr, t):
    import ctypes as C
    from oracle import orc
    w = orc.Waypoint()
    orc.lib().orc_primitive_evaluate(C.byref(pr), t, C.byref(w))
    return np.array(w.pos), list(w.acc)


def ellipsoids(ck, s13, i):
    """the n + 1 ellipsoids isFree tests on primitive (s13, U[i]): [(centre, C, (b1, b2, b3))]"""
    from tests import cloud_checker as K
    pr = primitive(ck, s13, i)
    r = ck.cloud.r
    n = n_of(pr, ck.dt, r)
    out = []
    for j in range(n + 1):
        d, acc = sample(pr, 0.0 if n == 0 else j * (ck.dt / n))
        Cm, b = K.ellipsoid_C((r, r, K.H_AXE), acc)
        out.append((d, np.array(Cm), tuple(np.array(x) for x in b)))
    return out


def _box(sc, margin):
    o, d = np.array(sc["ori"]), np.array(sc["dim"])
    return o + margin, o + d - margin


def surface_points(rng, ck, states, per_state=1):
    """points 1 -+ 1e-6 and 1 -+ 1e-3 (in the ellipsoid's norm) from the centre of ellipsoids that isFree tests"""
    pts = []
    for s13 in states:
        for _ in range(per_state):
            el = ellipsoids(ck, s13, int(rng.integers(len(ck.U))))
            d, Cm, _ = el[int(rng.integers(len(el)))]
            for f in (1 - 1e-6, 1 + 1e-6, 1 - 1e-3, 1 + 1e-3):
                u = rng.normal(size=3)
                pts.append(d + Cm @ (u / np.linalg.norm(u) * f))
    return np.array(pts)


def build_surface(sc, control, n_pts=None):
    rng = np.random.default_rng(1000 * sc["seed"] + control)
    r = sc["r"]
    lo, hi = _box(sc, min(0.6, 2 * r) if r < 1 else 3.0)
    states = random_states(rng, sc["n_states"], lo, hi, control, vel=sc["vel"])
    ck0 = checker(sc, control, [])
    near = surface_points(rng, ck0, states[::sc.get("near_every", 1)])
    lo, hi = _box(sc, -1.0)
    n_sc = sc.get("scatter", 300) if n_pts is None else max(n_pts - len(near), 0)
    pts = np.concatenate([near, rng.uniform(lo, hi, size=(n_sc, 3))])
    if n_pts is not None:
        pts = pts[rng.permutation(len(pts))[:n_pts]] if n_pts < len(pts) else pts
    return pts, states


def build_equator(sc, control):
    """8 x 8 resting states 1.6 m apart (60 kept); on two opposite primitives of each, a pair of points
    d + r (1 + e) (cos a b1 + sin a b2), e = -1e-7 and -1e-5, in the body frame of the t = dt sample, a within 0.4 rad of the
    direction of motion: inside that ellipsoid, on the rim of the radius filter, out of reach of every other sample"""
    rng = np.random.default_rng(1000 * sc["seed"] + control)
    o = np.array(sc["ori"])
    ck0 = checker(sc, control, [])
    r = sc["r"]
    states, pts = [], []
    cells = [(ix, iy) for ix in range(8) for iy in range(8)]
    for ix, iy in [cells[k] for k in rng.permutation(64)[:sc["n_states"]]]:
        p = o + np.array([1.6 * ix + 1.2, 1.6 * iy + 1.2, 1.0]) + np.r_[rng.uniform(-0.15, 0.15, size=2), rng.uniform(-0.3, 0.3)]
        s13 = np.zeros(13)
        s13[0:3] = p
        states.append(s13)
        nz = [i for i, u in enumerate(ck0.U) if np.any(u != 0)]
        i = nz[int(rng.integers(len(nz)))]
        opp = [k for k, u in enumerate(ck0.U) if np.array_equal(u, -ck0.U[i])][0]
        for k in (i, opp):
            el = ellipsoids(ck0, s13, k)
            assert len(el) == 2
            d, _, (b1, b2, b3) = el[1]
            m = ck0.U[k] / np.linalg.norm(ck0.U[k])
            a0 = math.atan2(float(m @ b2), float(m @ b1))
            for e in (-1e-7, -1e-5):
                a = a0 + rng.uniform(-0.4, 0.4)
                pts.append(d + r * (1 + e) * (math.cos(a) * b1 + math.sin(a) * b2))
    return np.array(pts), np.array(states)


def cell_of(x, r):
    """the device index's cell coordinate of a float32 coordinate: floor((double)x_f * inv_cell)"""
    inv = 1.0 / (float(np.float32(r)) * CELL_MARGIN)
    return math.floor(float(np.float32(x)) * inv)


FACE_CORNERS = ((-7, -5, -3), (-4, 3, -6), (5, -2, 2), (9, 8, 4), (0, 0, 0), (-1, 6, 1), (3, -9, -1), (-10, -10, -8))


def build_cell_faces(sc, control):
    """Eight cell corners k L (cell indices of both signs, and 0); at each, one point moved by -1, 0 or +1 float32 ulp per axis (a
    different combination per corner) and eight resting states, one per octant around it, 0.36 m away in x and y: the t = 0 ellipsoid
    just misses the point, the primitives towards it hold it, and it is found through a neighbour cell whenever the nudge and the octant
    disagree on an axis"""
    L = float(np.float32(sc["r"])) * CELL_MARGIN
    pts, states = [], []
    for c, corner in enumerate(FACE_CORNERS):
        x = np.array([np.float32(k * L) for k in corner], dtype=np.float32)
        nudge = [(c >> ax) & 1 for ax in range(3)]
        for ax in range(3):
            step = (1 if nudge[ax] else -1) if c < 7 else 0  # (the last corner keeps k L itself)
            if step:
                x[ax] = np.nextafter(x[ax], np.float32(np.inf * step))
        p = x.astype(np.float64)
        pts.append(p)
        for o in range(8):
            sg = np.array([1.0 if (o >> ax) & 1 else -1.0 for ax in range(3)])
            s13 = np.zeros(13)
            s13[0:3] = p + sg * np.array([0.36, 0.36, 0.02])
            states.append(s13)
    return np.array(pts), np.array(states)


def build_knife_edge(sc, control):
    """r = 0.625, VEL states (acceleration 0: the ellipsoid is axis-aligned) on a 2^-6 lattice, dt = 0.25, inputs of +-2 m/s: the
    primitive (2, 2, 0) tests the centres p and c = p + (0.5, 0.5, 0).  States 0..3: a point at exactly c + (r, 0, 0) /
    c + (0.375, 0.5, 0) (squared distance r^2 in float32: not a candidate of E2), at positive and at negative coordinates; states
    4..7: the same points one float32 ulp nearer to c"""
    base = [(2.0 + 5 / 64, 1.0 + 9 / 64), (-6.0 + 3 / 64, -4.0 - 7 / 64), (2.0 + 5 / 64, -4.0 - 7 / 64), (-6.0 + 3 / 64, 1.0 + 9 / 64)]
    offs = [(0.625, 0.0), (0.375, 0.5), (0.375, 0.5), (0.625, 0.0)]
    pts, states = [], []
    for inward in (False, True):
        for (bx, by), (ox, oy) in zip(base, offs):
            px = bx + (4.0 if inward else 0.0)
            s13 = np.zeros(13)
            s13[0:3] = (px, by, 0.0)
            cx, cy = px + 0.5, by + 0.5
            q = np.array([cx + ox, cy + oy, 0.0], dtype=np.float32)
            assert float(q[0]) == cx + ox and float(q[1]) == cy + oy
            if inward:
                q[0] = np.nextafter(q[0], np.float32(cx))
            pts.append(q.astype(np.float64))
            states.append(s13)
    return np.array(pts), np.array(states)


def build_index(sc, control):
    """a cloud of exactly n_pts points.  n_pts <= 8: every point 1e-3 inside an ellipsoid that a primitive of a different state tests;
    larger: the surface builder's cloud cut or filled to the size"""
    n = sc["n_pts"]
    if n > 8:
        return build_surface(sc, control, n_pts=n)
    rng = np.random.default_rng(1000 * sc["seed"] + control)
    lo, hi = _box(sc, 0.6)
    states = random_states(rng, sc["n_states"], lo, hi, control, vel=sc["vel"])
    ck0 = checker(sc, control, [])
    pts = []
    for k in range(n):
        el = ellipsoids(ck0, states[3 * k], int(rng.integers(len(ck0.U))))
        d, Cm, _ = el[-1]
        u = rng.normal(size=3)
        pts.append(d + Cm @ (u / np.linalg.norm(u) * (1 - 1e-3)))
    return np.array(pts), states


def build_copies(sc, control):
    """`copies` copies of one point that blocks a primitive (all in one bucket of the index), among a few dozen other points"""
    pts, states = build_surface(dict(sc, scatter=40), control)
    rng = np.random.default_rng(sc["seed"])
    return np.concatenate([pts[:50], np.repeat(pts[2:3], sc["copies"], axis=0), pts[50:]])[rng.permutation(len(pts) + sc["copies"])], states


NONFINITE = (math.nan, math.inf, -math.inf, 1e300, -1e300, 1e30, -1e30)


def build_nonfinite(sc, control, finite_only=False):
    """the surface cloud plus points with one, two or three coordinates that are NaN, +-inf, +-1e300 or +-1e30 and the others at the
    position of a state (where a finite point would block every primitive of it)"""
    pts, states = build_surface(sc, control)
    if finite_only:
        return pts, states
    bad = []
    for k, v in enumerate(NONFINITE):
        for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
            p = states[(len(bad)) % len(states), 0:3].copy()
            p[list(axes)] = v
            bad.append(p)
    bad = np.array(bad)
    rng = np.random.default_rng(sc["seed"])
    return np.concatenate([pts, bad])[rng.permutation(len(pts) + len(bad))], states


def _resting(p, vel=(0.0, 0.0, 0.0)):
    s13 = np.zeros(13)
    s13[0:3], s13[3:6] = p, vel
    return s13


def build_ceil_edge(sc, control):
    """VEL, r = 0.5, dt = 0.25: the input (4, 0, 0) has max_v dt / r = 2 exactly, ellipsoids at p, p + 0.5, p + 1.  A point 0.49 m
    beside the middle one blocks it; with n = 3 (a ceil that overshoots) no centre would be within r of it.  Every other state has the
    point at 0.51 m"""
    o = np.array(sc["ori"])
    pts, states = [], []
    for k in range(sc["n_states"]):
        p = o + np.array([1.0 + 1.25 * k, 2.0 + 0.5 * (k % 3), 1.5])
        states.append(_resting(p))
        pts.append(p + np.array([0.5, 0.49 if k % 2 == 0 else 0.51, 0.0]))
    return np.array(pts), np.array(states)


def build_long(sc, control):
    """VEL, r = 0.05, dt = 1: the input (13, 0, 0) has n = 260, 261 ellipsoids, more than one staging chunk of 256.  State k has a point
    0.04 m (even k: blocks) or 0.051 m (odd k: misses) beside ellipsoid j = 0, 128, 255, 256, 259, 260 of that primitive"""
    o = np.array(sc["ori"])
    pts, states = [], []
    for k, j in enumerate((0, 128, 255, 256, 259, 260)):
        p = o + np.array([1.0 + 0.1 * k, 0.5 + 0.5 * k, 1.0])
        states.append(_resting(p))
        pts.append(p + np.array([13.0 * j / 260.0, -0.04 if k % 2 == 0 else -0.051, 0.0]))
    return np.array(pts), np.array(states)


def build_pair_totals(sc, control):
    """VEL, r = 0.05, dt = 1, inputs (7.49, 0, 0): 151 ellipsoids, (0, 5.19, 0): 105, (0, -5.24, 0): 106.  States near the low y face lose
    the third input to the box (151 + 105 = 256 pairs: exactly one staging chunk), states near the high face the second (257: one pair
    in a second chunk).  Odd states have a point that only the last ellipsoid of the last primitive holds"""
    o, d = np.array(sc["ori"]), np.array(sc["dim"])
    pts, states = [], []
    for k in range(sc["n_states"]):
        low = k % 4 < 2
        p = o + np.array([0.5 + 1.0 * k, 1.5 + 0.1 * k if low else d[1] - 1.5 - 0.1 * k, 1.0])
        states.append(_resting(p))
        end = p + (np.array([0.0, 5.19, 0.0]) if low else np.array([0.0, -5.24, 0.0]))
        pts.append(end + np.array([0.0, 0.04 if low else -0.04, 0.0]) * (1.0 if k % 2 else 2.0))
    return np.array(pts), np.array(states)


def build_mid_box(sc, control):
    """ACC, dt = 0.2: a state 0.1 m inside a face of the box moving at 4 m/s towards it, input 40 m/s^2 away from it: the primitive
    starts and ends at the same position and is 0.2 m farther out at t = dt / 2, outside the box.  No point is near"""
    o, d = np.array(sc["ori"]), np.array(sc["dim"])
    c = o + d / 2
    states = [_resting((o[0] + d[0] - 0.1, c[1], c[2]), (4.0, 0.0, 0.0)), _resting((o[0] + 0.1, c[1], c[2]), (-4.0, 0.0, 0.0)),
              _resting((c[0], o[1] + d[1] - 0.1, c[2]), (0.0, 4.0, 0.0)), _resting((c[0], o[1] + 0.1, c[2]), (0.0, -4.0, 0.0)),
              _resting((o[0] + d[0] - 0.3, c[1], c[2]), (4.0, 0.0, 0.0)), _resting(c, (4.0, 0.0, 0.0))]
    return np.array([c + np.array([0.0, 0.0, 1.0])]), np.array(states)


def at(sc, rel):
    """the point at offset `rel` from the scene's box origin"""
    return tuple(float(o + x) for o, x in zip(sc["ori"], rel))


# 16 queries of the slot-reuse batch on the door scene (VEL, heur_ignore_dynamics, max_num = REUSE_MAX_NUM): reached, capped, no path
# (a start in the sealed closet) and start-is-goal, in mixed order, every fourth of another kind; offsets from the box origin
REUSE_MAX_NUM = 42
REUSE_QUERIES = (
    ((1.5, 0.8, 1.0), (10.5, 5.0, 1.0)), ((10.5, 1.5, 1.0), (1.5, 3.0, 1.0)), ((5.0, 3.0, 1.0), (9.5, 4.5, 1.0)), ((3.0, 3.0, 1.0), (3.5, 3.5, 1.0)),
    ((8.0, 5.5, 1.0), (2.0, 5.5, 1.0)), ((1.5, 5.2, 1.0), (10.5, 5.0, 1.0)), ((11.0, 1.0, 1.0), (4.0, 5.0, 1.0)), ((2.0, 1.0, 1.0), (8.0, 1.0, 1.0)),
    ((10.0, 2.0, 1.0), (10.5, 5.0, 1.0)), ((4.5, 0.6, 1.0), (7.5, 0.6, 1.0)), ((1.0, 1.0, 1.0), (10.5, 5.2, 1.0)), ((10.5, 5.0, 1.0), (1.5, 0.8, 1.0)),
    ((7.5, 5.5, 1.0), (7.0, 4.5, 1.0)), ((7.5, 0.8, 1.0), (1.5, 5.0, 1.0)), ((11.5, 0.5, 1.0), (11.5, 5.5, 1.0)), ((4.0, 5.5, 1.0), (8.5, 1.0, 1.0)),
)


def build_door(sc, control):
    """points every 0.1 m: a wall in the plane x = 6 with a doorway 2 < y < 4, and the walls x = 9, y < 3 and y = 3, x > 9 that seal the
    corner 9 < x < 12, 0 < y < 3 (the box closes its other two sides); coordinates relative to the box origin.  The states are for
    get_succ"""
    o = np.array(sc["ori"])
    g = lambda a, b: a + 0.1 * np.arange(int(round((b - a) / 0.1)) + 1)
    zs = g(0.0, 2.0)
    parts = [[(6.0, y, z) for y in np.r_[g(0.0, 2.0), g(4.0, 6.0)] for z in zs], [(9.0, y, z) for y in g(0.0, 3.0) for z in zs],
             [(x, 3.0, z) for x in g(9.1, 12.0) for z in zs]]
    pts = o + np.array([p for part in parts for p in part])
    rng = np.random.default_rng(1000 * sc["seed"] + control)
    lo, hi = _box(sc, 0.3)
    return pts, random_states(rng, sc["n_states"], lo, hi, control, vel=sc["vel"])


BUILDERS = dict(door=build_door, ceil_edge=build_ceil_edge, long=build_long, pair_totals=build_pair_totals, mid_box=build_mid_box,
                surface=build_surface, equator=build_equator, cell_faces=build_cell_faces, knife_edge=build_knife_edge, index=build_index,
                copies=build_copies, nonfinite=build_nonfinite)
_built = {}


def build(name, control):
    """(points, states) of scene `name` for one control kind: built once, shared by the tests, never modified"""
    if (name, control) not in _built:
        sc = SCENES[name]
        pts, states = BUILDERS[sc["build"]](sc, control)
        pts.setflags(write=False)
        states.setflags(write=False)
        _built[(name, control)] = (pts, states)
    return _built[(name, control)]
