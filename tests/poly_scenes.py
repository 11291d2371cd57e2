"""Named, seeded 2-D moving-obstacle scenes: one per regime poly_collide_all (mpl_ros_amd/csrc/mplx_poly_dev.h, switches
P1..P9 there) and its callers switch between.  TEST INFRASTRUCTURE ONLY.

A scene is a function of a seed and returns a Scene: one or more PolyWorld, the planner set-up (control kind, U, dt, v_max,
a_max, j_max, w), get_succ states (with the world each one is expanded in) and a few plans (world, start, goal, plan kwargs).
`expect` names the regime the scene is there for -- tests/test_poly_geometry.py restates every figure from the scene data and
the CPU checker alone and compares; `tags` says which further comparisons run on it (jrk, velsnp, shapes, lpa, heur).

Left out, because the reference leaves them undefined: an obstacle with an empty trajectory (Trajectory::evaluate of no
segments) and segments of negative duration.  A zero-duration segment is defined (it is never selected) and is in."""
import numpy as np

from mpl_ros_amd import poly_map as pm

ACC, JRK, VEL, SNP = pm.ACC, pm.JRK, pm.VEL, pm.SNP
U9 = pm.U9
STD_BOX = ((0.0, -5.0), (10.0, 10.0))


# ---------------------------------------------------------------- polyhedra: rows {px, py, nx, ny}
def ngon(n, r, rot=0.0, center=(0.0, 0.0)):
    """Regular n-gon of inradius r: normal k points at angle rot + 2 pi k / n, its hyperplane passes through center + r normal.
    A center further from the origin than the circumradius puts the obstacle's reference point outside the polygon."""
    rows = []
    for k in range(n):
        a = rot + 2.0 * np.pi * k / n
        nx, ny = float(np.cos(a)), float(np.sin(a))
        rows.append([center[0] + r * nx, center[1] + r * ny, nx, ny])
    return np.array(rows, dtype=np.float64)


def half_plane(angle, offset=0.0):
    """{x : n . x <= offset}, n at `angle`: one hyperplane, unbounded"""
    nx, ny = float(np.cos(angle)), float(np.sin(angle))
    return np.array([[offset * nx, offset * ny, nx, ny]], dtype=np.float64)


def slab(half_width, angle):
    """{x : |n . x| <= half_width}: two parallel hyperplanes, unbounded along the strip"""
    nx, ny = float(np.cos(angle)), float(np.sin(angle))
    return np.array([[half_width * nx, half_width * ny, nx, ny], [-half_width * nx, -half_width * ny, -nx, -ny]], dtype=np.float64)


def lattice(n, u_max):
    """n control inputs: the points of a 7 x 7 grid over [-u_max, u_max]^2, nearest to the origin first (ties: grid order)"""
    g = np.linspace(-u_max, u_max, 7)
    pts = np.array([(x, y) for x in g for y in g])
    order = np.argsort(np.round(np.hypot(pts[:, 0], pts[:, 1]), 9), kind="stable")
    return np.ascontiguousarray(pts[order[:n]])


def square_lattice(k, u_max):
    g = np.linspace(-u_max, u_max, k)
    return np.array([(x, y) for x in g for y in g])


class Scene:
    def __init__(self, name, worlds, states, world_of, plans, control=ACC, U=U9, dt=0.5, v_max=2.0, a_max=1.0, j_max=1.5, w=10.0, tags=(), expect=None):
        self.name, self.worlds, self.control, self.U = name, worlds, control, np.ascontiguousarray(U, dtype=np.float64)
        self.env = dict(dt=dt, v_max=v_max, a_max=a_max, j_max=j_max, w=w)
        self.states, self.world_of = np.ascontiguousarray(states, dtype=np.float64), np.asarray(world_of, dtype=np.int32)
        self.plans = plans            # [dict(world=, start=, goal=, kw=dict(eps=, max_expand=, ...))]
        self.tags = set(tags)
        self.expect = expect or {}
        assert len(self.states) == len(self.world_of) <= 200

    @property
    def n_u(self):
        return len(self.U)

    @property
    def dt(self):
        return self.env["dt"]


# ---------------------------------------------------------------- building blocks
def _pos(rng, W, margin=0.3, clear=()):
    lo, hi = W.ori + margin, W.ori + W.dim - margin
    for _ in range(1000):
        p = rng.uniform(lo, hi)
        if all(np.max(np.abs(p - np.array(c))) > r for c, r in clear):
            return p
    raise RuntimeError("no free position")


def scatter(rng, W, n_static, n_linear, n_nonlinear, dt, size=(0.25, 0.45), clear=(), poly=None, speed=0.4, n_seg=(2, 7), seg_dt=None, cov=(0.0, 0.1)):
    """random obstacles of the three kinds, kept off the `clear` squares ((center, half size)) at their first position"""
    poly = poly or (lambda: pm.rectangle(float(rng.uniform(*size)), float(rng.uniform(*size))))
    for _ in range(n_static):
        W.static.append(pm.StaticObstacle(poly(), _pos(rng, W, clear=clear)))
    for _ in range(n_linear):
        W.linear.append(pm.LinearObstacle(poly(), _pos(rng, W, clear=clear), rng.uniform(-speed, speed, 2), cov_v=float(rng.choice(cov))))
    for _ in range(n_nonlinear):
        n = int(rng.integers(*n_seg))
        us = U9[rng.integers(0, 9, n)] * 0.5
        segs = pm.acc_segs(_pos(rng, W, clear=clear), np.round(rng.uniform(-speed, speed, 2), 1), us, seg_dt or dt)
        W.nonlinear.append(pm.NonlinearObstacle(poly(), segs, start_t=float(rng.choice([0.0, 0.3, -0.5])), disappear_front=bool(rng.integers(0, 2)),
                                                disappear_back=bool(rng.integers(0, 2))))
    return W


def states_in(rng, W, n, dt, v=1.5, levels=8, lattice_share=8, t0=None):
    """n states inside world W's box: two-decimal positions (every lattice_share-th on the integer lattice: hyperplane-boundary
    cases), one-decimal velocities, node times t0 + k dt (t0: the world's start time)"""
    s = np.zeros((n, 9))
    s[:, 0:2] = W.ori + np.round(rng.uniform(0.02, 0.98, (n, 2)) * W.dim, 2)
    s[:, 2:4] = np.round(rng.uniform(-v, v, (n, 2)), 1)
    s[:, 8] = (W.start_t if t0 is None else t0) + rng.integers(0, levels, n) * dt
    k = n // lattice_share if lattice_share else 0
    s[:k, 0:2] = np.round(s[:k, 0:2])
    return s


def states_near(rng, W, n, dt, v=1.0, levels=6, reach=1.2):
    """n states within `reach` of an obstacle of W (at the obstacle's first position), so that blocked edges are common"""
    cs = [np.array(o.p) for o in W.static + W.linear] + [np.array([o.segs[0, 5], o.segs[0, 11]]) for o in W.nonlinear]
    s = states_in(rng, W, n, dt, v, levels, lattice_share=0)
    if cs:
        for i in range(n):
            c = cs[int(rng.integers(0, len(cs)))]
            p = np.round(c + rng.uniform(-reach, reach, 2), 2)
            s[i, 0:2] = np.minimum(np.maximum(p, W.ori + 0.01), W.ori + W.dim - 0.01)
    return s


def face_states(W, dt, t):
    """states on the four faces of the box, just outside them and at two corners"""
    (ox, oy), (dx, dy) = W.ori, W.dim
    mx, my = ox + dx / 2, oy + dy / 2
    pts = [(ox, my), (ox + dx, my), (mx, oy), (mx, oy + dy), (ox, oy), (ox + dx, oy + dy),
           (np.nextafter(ox, -np.inf), my), (np.nextafter(ox + dx, np.inf), my), (mx, oy - 1e-9), (mx, oy + dy + 1e-9), (ox - 0.2, my), (mx, oy + dy + 0.2)]
    s = np.zeros((len(pts), 9))
    s[:, 0:2] = pts
    s[:, 8] = t
    s[::2, 2] = 0.5
    s[1::2, 3] = -0.5
    return s


def plan(world, start, goal, t=None, v=(0.0, 0.0), **kw):
    s, g = np.zeros(9), np.zeros(9)
    s[0:2], s[2:4], s[8] = start, v, 0.0 if t is None else t
    g[0:2] = goal
    kw.setdefault("max_expand", 1500)
    return dict(world=world, start=s, goal=g, kw=kw)


def _mix(states_list):
    states = np.concatenate([s for _, s in states_list])
    world_of = np.concatenate([np.full(len(s), w, dtype=np.int32) for w, s in states_list])
    return states, world_of


# ---------------------------------------------------------------- obstacle count (P1)
def count_small(seed):
    """worlds of 0 and 1 obstacles"""
    rng = np.random.default_rng(seed)
    W0 = pm.PolyWorld(*STD_BOX)
    W1 = pm.PolyWorld(*STD_BOX, start_t=0.5)
    W1.nonlinear.append(pm.NonlinearObstacle(ngon(5, 0.8, 0.3), pm.acc_segs((5.0, 0.0), (0.2, -0.1), U9[[1, 7, 4]] * 0.5, 0.5), start_t=0.0))
    st, wo = _mix([(0, states_in(rng, W0, 20, 0.5)), (0, face_states(W0, 0.5, 0.0)), (1, states_near(rng, W1, 40, 0.5))])
    return Scene("count_small", [W0, W1], st, wo, [plan(0, (1.0, 0.0), (9.0, 0.5)), plan(1, (2.0, 0.0), (8.5, 0.0), t=0.5)], expect=dict(n_obs=[0, 1]))


def count_edge(seed):
    """63, 64 and 65 obstacles, the kinds mixed; the box off the origin"""
    rng = np.random.default_rng(seed)
    box = ((-37.3, 12.9), (10.0, 10.0))
    clear = [((-36.3, 17.9), 0.9), ((-28.3, 18.4), 0.9)]
    worlds = []
    for n in (63, 64, 65):
        W = pm.PolyWorld(*box, start_t=0.5)
        scatter(rng, W, n // 3, n // 3, n - 2 * (n // 3), 0.5, size=(0.15, 0.3), clear=clear)
        worlds.append(W)
    st, wo = _mix([(k, np.concatenate([states_in(rng, W, 20, 0.5), states_near(rng, W, 30, 0.5, reach=0.7)])) for k, W in enumerate(worlds)])
    plans = [plan(k, (-36.3, 17.9), (-28.3, 18.4), t=0.5, max_expand=3000) for k in range(3)]
    return Scene("count_edge", worlds, st, wo, plans, tags=("jrk", "lpa", "shapes", "heur"), expect=dict(n_obs=[63, 64, 65]))


def count_100(seed):
    """100 obstacles, crowded; the box far off the origin"""
    rng = np.random.default_rng(seed)
    box = ((1e3, -1e4), (12.0, 12.0))
    clear = [((1001.0, -9994.0), 0.9), ((1006.5, -9993.5), 0.9)]
    W = scatter(rng, pm.PolyWorld(*box), 40, 30, 30, 0.5, size=(0.2, 0.35), clear=clear)
    st, wo = _mix([(0, np.concatenate([states_in(rng, W, 40, 0.5), states_near(rng, W, 60, 0.5, reach=0.7), face_states(W, 0.5, 0.5)]))])
    return Scene("count_100", [W], st, wo, [plan(0, (1001.0, -9994.0), (1006.5, -9993.5), max_expand=3000)], tags=("velsnp",), expect=dict(n_obs=[100]))


# ---------------------------------------------------------------- segments per span (P2)
def seg_span(seed):
    """obstacle trajectories with segments of dt / 2, dt / 3, dt / 4 and dt / 10, started on and off the segment lattice; 50 segments;
    two trajectories of three short segments and a long one, over and over"""
    rng = np.random.default_rng(seed)
    dt = 0.5
    W = pm.PolyWorld(*STD_BOX)
    for k, div in enumerate((2, 3, 4, 10, 2, 3, 4, 10)):
        n = 50 if div == 10 else 6 * div
        us = U9[rng.integers(0, 9, n)] * 0.6
        p0 = (2.0 + 2.0 * (k % 4), -2.5 + 4.5 * (k // 4))
        segs = pm.acc_segs(p0, np.round(rng.uniform(-0.4, 0.4, 2), 1), us, dt / div)
        W.nonlinear.append(pm.NonlinearObstacle(ngon(6, 0.45, 0.2), segs, start_t=0.0 if k < 4 else 0.3, disappear_back=bool(k % 2)))
    # collide() accepts a root of a later segment only while it <= that segment's duration (it compares it + T, not it + traj_t, with
    # the segment's end): behind equal segments a fourth one never contributes, behind three short ones a long one does
    for k, st0 in enumerate((0.0, 0.3)):
        us = U9[rng.integers(0, 9, 24)] * 0.6
        segs = np.concatenate([pm.acc_segs((0.0, 0.0), (0.0, 0.0), [u], T) for u, T in zip(us, [dt / 10, dt / 10, dt / 10, dt] * 6)])
        p, v = np.array([4.0 + 3.0 * k, -0.3 + 0.8 * k]), np.array([0.3 - 0.5 * k, 0.2])
        for sg in segs:  # chain the segments: each starts where the one before ends
            sg[[5, 11]], sg[[4, 10]] = p, v
            u, T = sg[[3, 9]], sg[12]
            p, v = u / 2 * T * T + v * T + p, u * T + v
        W.nonlinear.append(pm.NonlinearObstacle(ngon(6, 0.45, 0.2), segs, start_t=st0))
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 150, dt, reach=0.9), states_in(rng, W, 30, dt)]))])
    plans = [plan(0, (0.5, -1.0), (9.5, 0.0), max_expand=1500), plan(0, (5.0, -4.5), (5.0, 4.5), max_expand=1500)]
    return Scene("seg_span", [W], st, wo, plans, tags=("jrk", "lpa", "shapes", "velsnp"), expect=dict(overlaps={3, 4, 5, 11}, max_n_seg=50, long_fourth=True))


# ---------------------------------------------------------------- LDS staging limits (P3)
def lds_limits(seed):
    """hyperplane sums of 256 and 257 (octagons, one 9-gon), segment sums of 256 and 257, all within 64 obstacles"""
    rng = np.random.default_rng(seed)
    box = ((1e5, 1e5), (12.0, 12.0))
    a, b = np.array([1e5 + 1.0, 1e5 + 6.0]), np.array([1e5 + 11.0, 1e5 + 6.5])
    clear = [(a, 0.9), (b, 0.9)]
    worlds = []
    for extra in (0, 1):  # 32 obstacles: 32 x 8 = 256 hyperplanes, or 31 x 8 + 9 = 257
        W = pm.PolyWorld(*box)
        polys = iter([ngon(8, float(rng.uniform(0.25, 0.4)), float(rng.uniform(0, 1))) for _ in range(31)] + [ngon(8 + extra, 0.35, 0.1)])
        scatter(rng, W, 12, 10, 10, 0.5, clear=clear, poly=lambda: next(polys))
        worlds.append(W)
    for extra in (0, 1):  # 8 trajectories: 8 x 32 = 256 segments, or 7 x 32 + 33 = 257
        W = pm.PolyWorld(*box)
        for k in range(8):
            n = 32 + (extra if k == 7 else 0)
            segs = pm.acc_segs(_pos(rng, W, clear=clear), np.round(rng.uniform(-0.3, 0.3, 2), 1), U9[rng.integers(0, 9, n)] * 0.4, 0.25)
            W.nonlinear.append(pm.NonlinearObstacle(ngon(4, 0.5, 0.4), segs, start_t=float(rng.choice([0.0, 0.3]))))
        worlds.append(W)
    st, wo = _mix([(k, np.concatenate([states_near(rng, W, 35, 0.5, reach=0.9), states_in(rng, W, 10, 0.5)])) for k, W in enumerate(worlds)])
    plans = [plan(k, a, b, max_expand=1200) for k in range(4)]
    return Scene("lds_limits", worlds, st, wo, plans, tags=("shapes",), expect=dict(hp_sum=[256, 257, 32, 32], seg_sum=[None, None, 256, 257]))


# ---------------------------------------------------------------- hyperplanes per obstacle (P4, P6)
def hp_counts(seed):
    """n_hp = 1, 2, 3, 15 (world 0: the dense list), 16 (world 1), 17 and 40 (world 2); a reference point outside its polygon, a
    duplicated hyperplane; normals off the axes, the three obstacle kinds"""
    rng = np.random.default_rng(seed)
    W0, W1, W2 = pm.PolyWorld(*STD_BOX), pm.PolyWorld(*STD_BOX), pm.PolyWorld(*STD_BOX, start_t=0.37)
    W0.static.append(pm.StaticObstacle(half_plane(1.4, 0.0), (5.0, -4.2)))                       # the strip below y ~ -4.2, tilted
    W0.linear.append(pm.LinearObstacle(slab(0.15, 0.3), (7.5, 0.0), (-0.2, 0.0), cov_v=0.0))      # a thin unbounded wall drifting left
    W0.static.append(pm.StaticObstacle(ngon(3, 0.5, 0.7), (3.0, 2.0)))
    W0.nonlinear.append(pm.NonlinearObstacle(ngon(15, 0.6, 0.11), pm.acc_segs((3.0, -1.5), (0.2, 0.1), U9[[5, 3, 8, 0]] * 0.5, 0.5), start_t=0.0))
    W0.static.append(pm.StaticObstacle(ngon(5, 0.5, 0.45, center=(2.0, 1.5)), (3.0, -0.5)))       # reference point 2.5 away from the pentagon at (5, 1)
    tri = ngon(3, 0.45, 1.9)
    W0.linear.append(pm.LinearObstacle(np.concatenate([tri, tri[1:2]]), (6.0, 3.0), (0.1, -0.3), cov_v=0.1))  # hyperplane 1 twice
    W1.static.append(pm.StaticObstacle(ngon(16, 0.7, 0.05), (5.0, 0.5)))
    W1.nonlinear.append(pm.NonlinearObstacle(ngon(16, 0.5, 0.2), pm.acc_segs((3.0, -2.0), (0.3, 0.2), U9[[7, 7, 1, 4, 2]] * 0.5, 0.5), start_t=0.3))
    W1.linear.append(pm.LinearObstacle(ngon(7, 0.5, 0.3), (7.0, 2.0), (-0.3, -0.2), cov_v=0.1))
    W2.static.append(pm.StaticObstacle(ngon(17, 0.7, 0.05), (4.0, 0.5)))
    W2.nonlinear.append(pm.NonlinearObstacle(ngon(40, 0.6, 0.01), pm.acc_segs((6.0, -2.0), (-0.2, 0.3), U9[[3, 5, 7, 1]] * 0.5, 0.5), start_t=0.0))
    W2.linear.append(pm.LinearObstacle(ngon(17, 0.45, 0.6), (7.0, 3.0), (-0.3, -0.3), cov_v=0.05))
    worlds = [W0, W1, W2]
    st, wo = _mix([(k, np.concatenate([states_near(rng, W, 50, 0.5, reach=1.0), states_in(rng, W, 10, 0.5)])) for k, W in enumerate(worlds)])
    plans = [plan(0, (1.0, 0.0), (9.0, 0.5)), plan(1, (1.0, 0.0), (9.0, 0.5)), plan(2, (1.0, 0.5), (9.0, 0.5), t=0.37)]
    return Scene("hp_counts", worlds, st, wo, plans, tags=("jrk", "lpa", "shapes", "heur"),
                 expect=dict(hp_max=[15, 16, 40], n_hp={1, 2, 3, 4, 5, 7, 15, 16, 17, 40}, unbounded=2))


# ---------------------------------------------------------------- index-space switches (P4, P8)
def _nu_scene(name, seed, U, n_obs, box=STD_BOX, tags=(), w=10.0, v_max=2.0, size=(0.2, 0.35), max_expand=3000, span=None, v=(0.0, 0.0), clear=None, **expect):
    rng = np.random.default_rng(seed)
    W = pm.PolyWorld(*box)
    a = W.ori + np.array([1.0, W.dim[1] / 2])
    b = W.ori + W.dim - np.array([1.0, W.dim[1] / 2]) if span is None else a + np.array([span, 0.5])
    scatter(rng, W, n_obs // 3, n_obs // 3, n_obs - 2 * (n_obs // 3), 0.5, size=size, clear=clear or [(a, 0.8), (b, 0.8)])
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 40, 0.5, reach=0.8), states_in(rng, W, 20, 0.5), face_states(W, 0.5, 0.0)]))])
    return Scene(name, [W], st, wo, [plan(0, a, b, v=v, max_expand=max_expand)], U=U, w=w, v_max=v_max, tags=tags, expect=dict(n_obs=[n_obs], n_u=len(U), **expect))


def nu_1(seed):
    """one control input (none: the robot coasts) along the middle of a 20 m x 3 m corridor, the obstacles starting off the middle"""
    return _nu_scene("nu_1", seed, np.array([[0.0, 0.0]]), 6, box=((-5.0, 2.0), (20.0, 3.0)), v=(1.0, 0.0), clear=[((x, 3.5), 0.8) for x in np.arange(-5.0, 15.5, 0.5)], pairs=6)


def nu_25(seed):
    """5 x 5 inputs with |u| <= 0.5, w = 0"""
    return _nu_scene("nu_25", seed, square_lattice(5, 0.5), 12, w=0.0, tags=("shapes",), span=3.0, v=(0.5, 0.0), max_expand=1000, pairs=300)


def nu_31(seed):
    """31 inputs x 33 obstacles = 1023 pairs: the largest pair list; helpers still allowed"""
    return _nu_scene("nu_31", seed, lattice(31, 1.0), 33, tags=("shapes",), span=4.0, pairs=1023)


def nu_32(seed):
    """32 inputs x 32 obstacles = 1024 pairs: no pair list, no helpers (the masks hold 31 hit bits)"""
    return _nu_scene("nu_32", seed, lattice(32, 1.0), 32, tags=("shapes",), span=4.0, pairs=1024)


def nu_32_full(seed):
    """32 inputs x 64 obstacles = 2048 pairs: every entry of the per-pair LDS arrays in use"""
    return _nu_scene("nu_32_full", seed, lattice(32, 1.0), 64, size=(0.15, 0.25), span=3.0, pairs=2048)


def items_edge(seed):
    """linear obstacles only (mode 2, never pruned): 14 inputs, all valid (v_max = -1, states well inside), x 73 hyperplanes = 1022
    items (the dense list's capacity) in world 0 and x 74 = 1036 (the rectangular index space) in world 1; pairs = 126"""
    rng = np.random.default_rng(seed)
    worlds = []
    for last in (9, 10):
        W = pm.PolyWorld((0.0, 0.0), (20.0, 20.0))
        for k in range(9):
            n = 8 if k < 8 else last
            W.linear.append(pm.LinearObstacle(ngon(n, float(rng.uniform(0.4, 0.7)), float(rng.uniform(0, 1))), rng.uniform((6, 6), (14, 14)), rng.uniform(-0.3, 0.3, 2),
                                              cov_v=float(rng.choice([0.0, 0.1]))))
        worlds.append(W)
    ss = []
    for k, W in enumerate(worlds):
        s = states_near(rng, W, 40, 0.5, v=1.0, reach=1.0)
        s[:, 0:2] = np.minimum(np.maximum(s[:, 0:2], 4.0), 16.0)
        ss.append((k, s))
    st, wo = _mix(ss)
    plans = [plan(k, (5.0, 10.0), (8.5, 10.5), max_expand=2500) for k in range(2)]
    return Scene("items_edge", worlds, st, wo, plans, U=lattice(14, 1.0), v_max=-1.0, expect=dict(n_u=14, pairs=126, items=[1022, 1036], all_valid=True))


# ---------------------------------------------------------------- PolyObs::fast off (P5)
def _fast_world(rng, variants):
    W = pm.PolyWorld(*STD_BOX)
    for k, variant in enumerate(variants):
        p0 = (2.5 + 1.6 * (k % 4), -2.0 + 3.5 * (k // 4))
        segs = pm.acc_segs(p0, (0.2, 0.1 * (k % 3 - 1)), U9[[7, 5, 1, 3, 8, 0]] * 0.5, 0.5)
        if variant == "zero_T":      # a zero-duration segment in the middle (never selected)
            z = segs[3].copy()
            z[12] = 0.0
            segs = np.concatenate([segs[:3], z[None], segs[3:]])
        elif variant == "neg_zero":  # -0.0 leading coefficients
            segs[:, [0, 1, 2, 6, 7, 8]] = -0.0
        elif variant == "jrk_seg":   # one cubic segment, continuing segment 2's end state
            j = pm.jrk_segs((segs[3, 5], segs[3, 11]), (segs[3, 4], segs[3, 10]), (0.2, -0.1), [(0.4, -0.3)], 0.5)
            segs = np.concatenate([segs[:3], j, segs[4:]])
        W.nonlinear.append(pm.NonlinearObstacle(ngon(6, 0.5, 0.25), segs, start_t=float(rng.choice([0.0, 0.3])), disappear_back=bool(k % 2)))
    return W


def fast_off(seed):
    """trajectories that lose PolyObs::fast (a zero-duration segment, -0.0 leading coefficients) beside the same trajectories with it"""
    rng = np.random.default_rng(seed)
    W = _fast_world(rng, ["zero_T", "plain", "neg_zero", "plain", "zero_T", "neg_zero", "plain", "plain"])
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 120, 0.5, reach=0.9), states_in(rng, W, 20, 0.5)]))])
    plans = [plan(0, (0.5, -1.0), (9.5, 0.0)), plan(0, (0.5, 2.0), (9.5, -2.5))]
    return Scene("fast_off", [W], st, wo, plans, tags=("shapes",), expect=dict(fast=[0, 1, 0, 1, 0, 0, 1, 1], high_degree=False))


def fast_mixed(seed):
    """an ACC trajectory with one JRK segment in it (the whole launch turns to the general solve) beside plain ACC trajectories"""
    rng = np.random.default_rng(seed)
    W = _fast_world(rng, ["jrk_seg", "plain", "plain", "jrk_seg", "zero_T", "plain"])
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 100, 0.5, reach=0.9), states_in(rng, W, 20, 0.5)]))])
    plans = [plan(0, (0.5, -1.0), (9.5, 0.0), max_expand=800)]
    return Scene("fast_mixed", [W], st, wo, plans, tags=("jrk", "shapes"), expect=dict(fast=[0, 1, 1, 0, 0, 1], high_degree=True))


# ---------------------------------------------------------------- presence flags
def presence(seed):
    """disappear_front / disappear_back in the four combinations; node times before, at 0, inside, at total_t and after the trajectory"""
    rng = np.random.default_rng(seed)
    W = pm.PolyWorld(*STD_BOX)
    for k, (front, back) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        segs = pm.acc_segs((2.0 + 2.0 * k, -2.0), (0.0, 1.0), [(0.0, 0.0)] * 3, 0.5)  # 1.5 s straight up from y = -2 to y = -0.5
        W.nonlinear.append(pm.NonlinearObstacle(pm.rectangle(0.5), segs, start_t=-1.0, disappear_front=front, disappear_back=back))
    ss = []
    for t in (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5):  # traj_t = t - 1: -1, -0.5, 0 (= start), 0.5, 1, 1.5 (= total_t), 2, 2.5
        for k in range(4):
            for y in (-2.0, -1.2, -0.5, 0.3):  # at the clamped start, on the way, at the clamped end, just above
                ss.append([2.0 + 2.0 * k + 0.7, y, -0.6, 0.0, 0, 0, 0, 0, t])
    ss = np.array(ss)
    st, wo = _mix([(0, ss), (0, states_in(rng, W, 30, 0.5))])
    plans = [plan(0, (0.5, -1.2), (9.5, -1.2)), plan(0, (0.5, -1.2), (9.5, -1.2), t=2.0)]
    return Scene("presence", [W], st, wo, plans, expect=dict(traj_times={-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5}, total_t=1.5))


# ---------------------------------------------------------------- linear obstacles
def linear(seed):
    """v = 0; cov_v 0, 0.1 and negative (the polygon has shrunk to nothing from t = 2 on)"""
    rng = np.random.default_rng(seed)
    W = pm.PolyWorld(*STD_BOX)
    W.linear.append(pm.LinearObstacle(pm.rectangle(0.5), (3.0, 0.0), (0.0, 0.0), cov_v=0.0))
    W.linear.append(pm.LinearObstacle(ngon(5, 0.4, 0.3), (5.0, 2.0), (0.0, 0.0), cov_v=0.1))
    W.linear.append(pm.LinearObstacle(pm.rectangle(0.5), (5.0, -2.0), (0.0, 0.0), cov_v=-0.25))
    W.linear.append(pm.LinearObstacle(ngon(6, 0.5, 0.2), (7.0, 0.5), (-0.3, 0.2), cov_v=-0.25))
    W.linear.append(pm.LinearObstacle(pm.rectangle(0.3, 0.6), (8.0, -3.0), (-0.5, 0.4), cov_v=0.1))
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 110, 0.5, reach=0.9, levels=10), states_in(rng, W, 20, 0.5)]))])
    s = st[:12]
    s[:, 0:2], s[:, 2:4] = (5.0, -2.0), 0.0           # on the shrinking square's centre: blocked until t = 2 (within eps), free after
    s[:, 8] = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 1.5, 2.0, 2.5, 4.0]
    plans = [plan(0, (0.5, 0.0), (9.5, 0.0)), plan(0, (0.5, 0.0), (9.5, 0.0), t=3.0)]
    return Scene("linear", [W], st, wo, plans, tags=("velsnp",), expect=dict(cov_v={0.0, 0.1, -0.25}, v_zero=3))


# ---------------------------------------------------------------- time, box
def _time_scene(name, seed, dt, start_t, box, tags=(), n_obs=9, v_max=2.0, plan_kw=None, plan_t=None, cov=(0.0, 0.1), span=None, **expect):
    rng = np.random.default_rng(seed)
    W = pm.PolyWorld(*box, start_t=start_t)
    a = W.ori + np.array([0.4, W.dim[1] / 2])
    b = W.ori + W.dim - np.array([0.4, W.dim[1] / 2]) if span is None else a + np.array([span, 0.3])
    scatter(rng, W, n_obs // 3, n_obs // 3, n_obs - 2 * (n_obs // 3), dt, size=(0.08, 0.12) if min(W.dim) < 2 else (0.2, 0.35), clear=[(a, 0.3), (b, 0.3)] if min(W.dim) < 2 else [(a, 0.8), (b, 0.8)],
            speed=0.1 if min(W.dim) < 2 else 0.4, cov=cov)
    reach = 0.3 if min(W.dim) < 2 else 0.8
    below = states_in(rng, W, 20, dt, t0=start_t - 3 * dt)              # node times below the world's start time (and around it)
    off = states_near(rng, W, 20, dt, reach=reach)
    off[:, 8] += 0.013                                                   # off the time lattice
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 60, dt, reach=reach), states_in(rng, W, 20, dt), below, off, face_states(W, dt, start_t)]))])
    plans = [plan(0, a, b, t=start_t if plan_t is None else plan_t, **(plan_kw or {}))]
    return Scene(name, [W], st, wo, plans, dt=dt, v_max=v_max, tags=tags, expect=dict(dt=dt, start_t=start_t, **expect))


def time_dt025(seed):
    """dt 0.25, world start time 0.37, a 20 m x 3 m box off the origin"""
    return _time_scene("time_dt025", seed, 0.25, 0.37, ((-37.3, 12.9), (20.0, 3.0)), plan_kw=dict(eps=2.0, max_expand=2500), span=3.5)


def time_dt1(seed):
    """dt 1.0, world start time -2.0, the plan starting at t = 0 (two levels into the world's time)"""
    return _time_scene("time_dt1", seed, 1.0, -2.0, ((1e3, -1e4), (10.0, 10.0)), plan_t=0.0, tags=("heur",))


def time_dt03(seed):
    """dt 0.3, world start time 1e3, a 1.5 m x 1.5 m box at (1e5, 1e5).  The plan starts at t = 0: t_rel = -1000, below every cache
    level; a second one at t = 1019.5: t_rel / dt = 65, above every level"""
    S = _time_scene("time_dt03", seed, 0.3, 1e3, ((1e5, 1e5), (1.5, 1.5)), plan_t=0.0, v_max=1.0, cov=(0.0, 0.0), cache_level=False)
    p = S.plans[0]
    S.plans.append(dict(world=0, start=p["start"].copy(), goal=p["goal"].copy(), kw=dict(p["kw"])))
    S.plans[1]["start"][8] = 1019.5
    S.tags.add("shapes")
    return S


def deep(seed):
    """dt 0.1, v_max 1, eps 2 across 8.5 m of a lightly obstructed world: a path of more than 64 time levels (P7: no cache level
    beyond the 64th)"""
    rng = np.random.default_rng(seed)
    W = pm.PolyWorld(*STD_BOX)
    clear = [((0.75, 0.0), 0.8), ((9.25, 0.0), 0.8)]
    scatter(rng, W, 2, 2, 2, 0.1, clear=clear, seg_dt=0.5, n_seg=(8, 16))
    W.static.append(pm.StaticObstacle(pm.rectangle(0.3), (5.0, -0.2)))  # on the straight line; the LPA* test moves it off
    st, wo = _mix([(0, np.concatenate([states_near(rng, W, 60, 0.1, v=0.9, reach=0.7, levels=100), states_in(rng, W, 20, 0.1, v=0.9, levels=100)]))])
    plans = [plan(0, (0.75, 0.0), (9.25, 0.0), eps=2.0, max_expand=6000)]
    return Scene("deep", [W], st, wo, plans, dt=0.1, v_max=1.0, tags=("lpa", "shapes"), expect=dict(min_levels=65))


# ---------------------------------------------------------------- cache tags
def tags(seed):
    """four worlds of equal size and start time, different obstacles: queries that share a workgroup (fewer slots than queries)
    leave each other's prepared obstacles in the cache at the same time levels"""
    rng = np.random.default_rng(seed)
    clear = [((1.0, 0.0), 0.8), ((9.0, 0.0), 0.8)]
    worlds = [scatter(rng, pm.PolyWorld(*STD_BOX), 3, 3, 4, 0.5, clear=clear) for _ in range(4)]
    st, wo = _mix([(k, states_near(rng, W, 30, 0.5, reach=0.8)) for k, W in enumerate(worlds)])
    plans = [plan(k % 4, (1.0, 0.0), (9.0, 0.0), max_expand=1000) for k in range(8)]
    return Scene("tags", worlds, st, wo, plans, tags=("shapes",), expect=dict(n_obs=[10, 10, 10, 10], equal_start_t=True))


# ---------------------------------------------------------------- knife edges
def knife(seed):
    """obstacle faces on the lattice the states sit on (hyperplane roots at exactly it = 0 and it = T, points within the inside
    tolerance of a face), and obstacles at the pruning distance of a node: one just inside it, one just outside"""
    rng = np.random.default_rng(seed)
    W = pm.PolyWorld(*STD_BOX)
    sq = pm.rectangle(0.5)
    W.static.append(pm.StaticObstacle(sq, (3.0, 0.0)))      # faces x = 2.5, 3.5, y = +-0.5
    W.static.append(pm.StaticObstacle(sq, (6.0, 2.0)))      # faces x = 5.5, 6.5, y = 1.5, 2.5
    W.linear.append(pm.LinearObstacle(sq, (6.0, -2.0), (0.0, 0.0), cov_v=0.0))
    W.nonlinear.append(pm.NonlinearObstacle(sq, pm.acc_segs((8.0, 0.0), (0.0, 0.0), [(0.0, 0.0)] * 4, 0.5), start_t=0.0))  # standing at (8, 0)
    # pruning (P6): a node at rest at (1, 3), dt 0.5, |u| 1: rx = 0.125 + (radius + 1e-6) + 1e-6 with radius = |(0.5, 0.5)|
    rx = 0.5 * 1.0 * 0.25 + (float(np.hypot(0.5, 0.5)) + 1e-6) + 1e-6
    W.static.append(pm.StaticObstacle(sq, (1.0 + rx - 1e-9, 3.0)))
    W.static.append(pm.StaticObstacle(sq, (1.0, 3.0 - rx - 1e-9)))
    W.static.append(pm.StaticObstacle(sq, (1.0, 4.2)))  # face y = 3.7: a node at rest at y = 3.575 reaches it with u_y = 1 at the very end of the primitive
    ss = []
    for x, y, vx, vy in [(2.0, 0.0, 1.0, 0.0), (2.0, 0.0, 0.0, 0.0), (2.5, 0.0, -1.0, 0.0), (2.5, 1.0, 0.0, -1.0), (2.0, 0.5, 1.0, 0.0), (2.0, -0.5, 1.0, 0.0),
                         (2.0, 0.5 + 1e-10, 1.0, 0.0), (2.0, 0.5 + 2e-10, 1.0, 0.0), (2.5 - 1e-10, 0.0, -1.0, 0.0), (2.5 - 2e-10, 1.0, -1.0, 0.0), (4.0, 0.0, -1.0, 0.0),
                         (3.5, 0.5, 0.5, 0.5), (5.0, 2.0, 1.0, 0.0), (6.0, 1.0, 0.0, 1.0), (6.0, 3.0, 0.0, -1.0), (5.0, -2.0, 1.0, 0.0), (6.0, -3.0, 0.0, 1.0), (7.0, 0.0, 1.0, 0.0),
                         (7.0, 0.5, 1.0, 0.0), (8.0, 1.0, 0.0, -1.0), (1.0, 3.0, 0.0, 0.0), (1.0, 3.0, 0.5, 0.0), (1.0, 3.0, 0.0, -0.5), (1.0, 3.0, 1.0, -1.0), (1.2, 3.0, 1.0, 0.0),
                         (1.0, 3.2, 0.0, 0.0), (1.0, 3.2, 0.0, 1.0), (1.0, 3.45, 0.0, 0.5), (1.0, 3.575, 0.0, 0.0), (1.0, 3.575, 0.0, 0.25)]:
        for t in (0.0, 1.0):
            ss.append([x, y, vx, vy, 0, 0, 0, 0, t])
    st, wo = _mix([(0, np.array(ss)), (0, states_in(rng, W, 40, 0.5, lattice_share=1))])
    plans = [plan(0, (1.0, 0.0), (9.5, 0.0)), plan(0, (1.0, 3.0), (9.0, -3.0))]
    return Scene("knife", [W], st, wo, plans, tags=("velsnp",), expect=dict(prune_edge=rx))


SCENES = {f.__name__: f for f in (count_small, count_edge, count_100, seg_span, lds_limits, hp_counts, nu_1, nu_25, nu_31, nu_32, nu_32_full, items_edge,
                                  fast_off, fast_mixed, presence, linear, time_dt025, time_dt1, time_dt03, deep, tags, knife)}
SEED = 2024
JRK_REACH, JRK_CAP = 2.0, 1200
_made = {}


def get(name):
    """the scene of the fixed seed, built once per process"""
    if name not in _made:
        _made[name] = SCENES[name](SEED + sorted(SCENES).index(name))
        assert _made[name].name == name
    return _made[name]


def with_control(S, control):
    """the scene under another control kind: same worlds and plans, the states given the acceleration (JRK, SNP) and jerk (SNP)
    the kind carries (seeded per scene)"""
    rng = np.random.default_rng(SEED + 7 * control + sorted(SCENES).index(S.name))
    st = S.states.copy()
    if control in (JRK, SNP):
        st[:, 4:6] = np.round(rng.uniform(-1, 1, (len(st), 2)), 1)
    if control == SNP:
        st[:, 6:8] = np.round(rng.uniform(-1, 1, (len(st), 2)), 1)
    # a JRK / SNP state space grows much faster (position, velocity and acceleration in the key): the goal is brought to JRK_REACH
    # of the start, on the line to the scene's goal, so that plans are found within a cap the CPU checker runs in a second or two
    # (VEL / SNP variants get the same plans but never use them: the search runs ACC or JRK states only)
    plans = []
    keep = S.plans[-2:] if len({p["world"] for p in S.plans[-2:]}) == 2 else S.plans[-1:]
    for p in keep:  # (the last plan of the last two worlds: the checker needs seconds for each)
        d = p["goal"][0:2] - p["start"][0:2]
        g = p["goal"].copy()
        g[0:2] = p["start"][0:2] + d * min(1.0, JRK_REACH / float(np.hypot(*d)))
        plans.append(dict(world=p["world"], start=p["start"], goal=g, kw=dict(p["kw"], max_expand=min(p["kw"]["max_expand"], JRK_CAP))))
    T = Scene(S.name, S.worlds, st, S.world_of, plans, control=control, U=S.U, tags=S.tags, expect=S.expect, **S.env)
    return T
