"""Named, seeded 3-D moving-obstacle scenes: one per code path of p3_collide_all (mpl_ros_amd/csrc/mplx_poly3.h), its two
callers and the host code of mplx_poly3.hip that no world of tests/test_poly_map3d.py reaches.  TEST INFRASTRUCTURE ONLY.

Shaped like tests/poly_scenes.py (the Scene class is that one): a scene is a function of a seed and returns one or more
PolyWorld3D, the planner set-up, at most 200 get_succ states (13 columns: pos3 vel3 acc3 jrk3 t) with the world each one is
expanded in, and 2-4 plans.  `expect` names the regime -- tests/test_poly3_geometry.py restates every figure from the scene
data and the CPU checker alone; `tags` says which further comparisons run on it (jrk, velsnp, heur, tolvel).

Left out, for the reason poly_scenes.py gives (the reference leaves them undefined): an obstacle with an empty trajectory and
segments of negative duration."""
import numpy as np

from mpl_ros_amd import poly_map3d as p3
from tests.poly_scenes import Scene

VEL, ACC, JRK, SNP = p3.VEL, p3.ACC, p3.JRK, p3.SNP
U27 = p3.control_lattice(1.0, 1)
U7 = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float64)
STD_BOX = ((0.0, -5.0, 0.0), (10.0, 10.0, 4.0))
ENV = dict(dt=0.5, v_max=2.0, a_max=1.5, j_max=2.0, w=10.0)
BLOCK = 256  # lanes of the 3-D kernels: a lane's second trip through a loop starts at this index


# ---------------------------------------------------------------- polyhedra: rows {px, py, pz, nx, ny, nz}
def planes(normals, r, center=(0.0, 0.0, 0.0)):
    """one hyperplane per normal (normalised here), through center + r n.  A center further away than the shape is wide puts the
    obstacle's reference point outside its shape."""
    n = np.array(normals, dtype=np.float64)
    n = n / np.linalg.norm(n, axis=1)[:, None]
    return np.ascontiguousarray(np.concatenate([np.array(center) + r * n, n], axis=1))


def octahedron(r):
    return planes([(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], r)


def icosahedron(r, center=(0.0, 0.0, 0.0)):
    """20 tilted faces: the normals are the vertices of a dodecahedron"""
    f = (1.0 + 5.0 ** 0.5) / 2.0
    ns = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for a in (-1, 1):
        for b in (-1, 1):
            ns += [(0.0, a / f, b * f), (a / f, b * f, 0.0), (a * f, 0.0, b / f)]
    return planes(ns, r, center)


def half_space(normal, offset=0.0):
    return planes([normal], offset)


def slab(normal, half_width):
    return planes([normal, tuple(-np.array(normal, dtype=np.float64))], half_width)


def rand_poly(rng, size):
    k = int(rng.integers(0, 3))
    if k == 0:
        return p3.box(*[float(x) for x in rng.uniform(size[0], size[1], 3)])
    return octahedron(float(rng.uniform(*size)) * 1.4) if k == 1 else icosahedron(float(rng.uniform(*size)))


# ---------------------------------------------------------------- building blocks
def _pos(rng, W, margin=0.3, clear=()):
    lo, hi = W.ori + np.minimum(margin, W.dim / 4), W.ori + W.dim - np.minimum(margin, W.dim / 4)
    for _ in range(2000):
        p = rng.uniform(lo, hi)
        if all(np.max(np.abs(p - np.array(c))) > r for c, r in clear):
            return p
    raise RuntimeError("no free position")


def scatter(rng, W, n_static, n_linear, n_nonlinear, dt, size=(0.25, 0.45), clear=(), speed=0.4, n_seg=(2, 7), cov=(0.0, 0.1), segs=None, poly=None, line=None):
    """random obstacles of the three kinds (static first, then linear, then nonlinear), kept off the `clear` cubes ((center, half
    size)) at their first position.  segs(p0, v0): the trajectory of a nonlinear obstacle (default: ACC segments of dt).
    line = (a, b): the first static obstacle is put in the middle of that line and the first linear one crosses it a second
    after the world's start, so that a plan from a to b has to go round them"""
    poly = poly or (lambda: rand_poly(rng, size))
    for _ in range(n_static):
        W.static.append(p3.StaticObstacle3D(poly(), _pos(rng, W, clear=clear)))
    for _ in range(n_linear):
        W.linear.append(p3.LinearObstacle3D(poly(), _pos(rng, W, clear=clear), rng.uniform(-speed, speed, 3), cov_v=float(rng.choice(cov))))
    for _ in range(n_nonlinear):
        p0, v0 = _pos(rng, W, clear=clear), np.round(rng.uniform(-speed, speed, 3), 1)
        sg = segs(p0, v0) if segs else p3.acc_segs(p0, v0, U27[rng.integers(0, 27, int(rng.integers(*n_seg)))] * 0.5, dt)
        W.nonlinear.append(p3.NonlinearObstacle3D(poly(), sg, start_t=float(rng.choice([0.0, 0.3, -0.5])), disappear_front=bool(rng.integers(0, 2)),
                                                  disappear_back=bool(rng.integers(0, 2))))
    if line is not None:
        a, b = np.array(line[0], float), np.array(line[1], float)
        if W.static:
            W.static[0].p = a + 0.5 * (b - a) + (0.0, 0.1, -0.1)
        if W.linear:
            W.linear[0].p = (a + 0.65 * (b - a) + (0.0, 0.5, 0.2)) - W.linear[0].v * 1.0
    return W


def obstacles(W):
    return W.static + W.linear + W.nonlinear


def states_in(rng, W, n, dt, v=1.5, levels=8, lattice_share=8, t0=None):
    """n states inside W's box: two-decimal positions (every lattice_share-th on the integer lattice), one-decimal velocities,
    node times t0 + k dt (t0: the world's start time)"""
    s = np.zeros((n, 13))
    s[:, 0:3] = W.ori + np.round(rng.uniform(0.02, 0.98, (n, 3)) * W.dim, 2)
    s[:, 3:6] = np.round(rng.uniform(-v, v, (n, 3)), 1)
    s[:, 12] = (W.start_t if t0 is None else t0) + rng.integers(0, levels, n) * dt
    k = n // lattice_share if lattice_share else 0
    s[:k, 0:3] = np.minimum(np.maximum(np.round(s[:k, 0:3]), W.ori), W.ori + W.dim)
    return s


def first_pos(o):
    return np.array(o.segs[0, [5, 11, 17]]) if hasattr(o, "segs") else np.array(o.p)


def states_near(rng, W, n, dt, v=1.0, levels=6, reach=1.0, only=None):
    """n states within `reach` of an obstacle of W (at the obstacle's first position), so that blocked edges are common"""
    s = states_in(rng, W, n, dt, v, levels, lattice_share=0)
    obs = obstacles(W) if only is None else only
    for i in range(n if obs else 0):
        c = first_pos(obs[int(rng.integers(0, len(obs)))])
        p = np.round(c + rng.uniform(-reach, reach, 3), 2)
        s[i, 0:3] = np.minimum(np.maximum(p, W.ori + 0.01), W.ori + W.dim - 0.01)
    return s


def face_states(W, t):
    """states on the six faces of the box, 1e-10 either side of each, at two corners and well outside"""
    lo, hi, mid = W.ori, W.ori + W.dim, W.ori + W.dim / 2
    pts = []
    for ax in range(3):
        for edge in (lo[ax], hi[ax]):
            for d in (0.0, -1e-10, 1e-10):
                p = mid.copy()
                p[ax] = edge + d
                pts.append(p)
    pts += [lo.copy(), hi.copy(), mid - W.dim, mid + W.dim]
    s = np.zeros((len(pts), 13))
    s[:, 0:3] = pts
    s[:, 12] = t
    s[::2, 3] = 0.5
    s[1::2, 5] = -0.5
    return s


def plan(world, start, goal, t=None, v=(0.0, 0.0, 0.0), gv=(0.0, 0.0, 0.0), **kw):
    s, g = np.zeros(13), np.zeros(13)
    s[0:3], s[3:6], s[12] = start, v, 0.0 if t is None else t
    g[0:3], g[3:6] = goal, gv
    kw.setdefault("max_expand", 400)
    kw.setdefault("eps", 2.0)
    return dict(world=world, start=s, goal=g, kw=kw)


def _mix(states_list, shuffle=None):
    states = np.concatenate([s for _, s in states_list])
    world_of = np.concatenate([np.full(len(s), w, dtype=np.int32) for w, s in states_list])
    if shuffle is not None:
        order = shuffle.permutation(len(states))
        states, world_of = states[order], world_of[order]
    return states, world_of


def scene(name, worlds, states, world_of, plans, control=ACC, U=U27, tags=(), expect=None, **env):
    return Scene(name, worlds, states, world_of, plans, control=control, U=U, tags=tags, expect=expect, **dict(ENV, **env))


A, B = np.array([1.0, 0.0, 2.0]), np.array([3.5, 0.5, 2.0])  # the usual plan end points of the standard box
CLEAR = [(A, 0.8), (B, 0.8)]


def _std_states(rng, W, n_near=110, n_in=40, dt=0.5, reach=0.9):
    return np.concatenate([states_near(rng, W, n_near, dt, reach=reach), states_in(rng, W, n_in, dt)])


# ---------------------------------------------------------------- the pair loop and the start-point loop
def pairs_one_pass(seed):
    """27 inputs x 9 obstacles = 243 pairs: the last size at which no lane takes a second trip"""
    rng = np.random.default_rng(seed)
    W = scatter(rng, p3.PolyWorld3D(*STD_BOX), 3, 3, 3, 0.5, clear=CLEAR, line=(A, B))
    st, wo = _mix([(0, _std_states(rng, W))])
    plans = [plan(0, A, B), plan(0, A, B + (0.0, -1.0, 0.5), gv=(0.5, 0.0, 0.0))]
    return scene("pairs_one_pass", [W], st, wo, plans, tags=("heur", "tolvel"), expect=dict(n_obs=[9], pairs=[243]))


def pairs_strided(seed):
    """27 x 10 = 270 and 27 x 11 = 297 pairs: lanes 0..13 (0..40) take a second trip, and the pairs of such a lane lie in two
    primitives (e / n_obs differs between its trips).  (32 x 9 = 288 is the scene nu_32.)"""
    rng = np.random.default_rng(seed)
    worlds = [scatter(rng, p3.PolyWorld3D(*STD_BOX, start_t=0.5 * k), 3, 3 + k, 4, 0.5, clear=CLEAR, line=(A, B)) for k in (0, 1)]
    st, wo = _mix([(k, _std_states(rng, W, 70, 30)) for k, W in enumerate(worlds)])
    plans = [plan(0, A, B), plan(1, A, B, t=0.5)]
    return scene("pairs_strided", worlds, st, wo, plans, tags=("jrk", "velsnp"), expect=dict(n_obs=[10, 11], pairs=[270, 297]))


def _crowd(rng, n, start_t=0.0, size=(0.12, 0.22)):
    return scatter(rng, p3.PolyWorld3D(*STD_BOX, start_t=start_t), n // 3, n // 3, n - 2 * (n // 3), 0.5, size=size, clear=[(A, 0.6), (B, 0.6)], speed=0.3, line=(A, B))


def obs_300(seed):
    """300 obstacles of the three kinds in one world: the start-point loop strides (lanes 0..43 test two obstacles), 8 100 pairs"""
    rng = np.random.default_rng(seed)
    W = _crowd(rng, 300)
    s = _std_states(rng, W, 110, 40, reach=0.5)
    late = obstacles(W)[BLOCK:]  # states where an obstacle beyond the 256th is at t = 0: only a lane's second trip sees it
    s[:len(late), 0:3], s[:len(late), 12] = [first_pos(o) for o in late], 0.0
    st, wo = _mix([(0, s)])
    plans = [plan(0, A, B, max_expand=150), plan(0, A, A + (2.0, -0.5, 0.5), max_expand=150)]
    return scene("obs_300", [W], st, wo, plans, expect=dict(n_obs=[300], pairs=[8100], late_start_hit=True))


def obs_0_1(seed):
    """worlds with no obstacle and with one"""
    rng = np.random.default_rng(seed)
    W0 = p3.PolyWorld3D(*STD_BOX)
    W1 = p3.PolyWorld3D(*STD_BOX, start_t=0.5)
    W1.nonlinear.append(p3.NonlinearObstacle3D(icosahedron(0.8), p3.acc_segs((3.0, 0.2, 2.0), (0.2, -0.1, 0.0), U27[[1, 7, 4]] * 0.5, 0.5), start_t=0.0))
    st, wo = _mix([(0, states_in(rng, W0, 20, 0.5)), (0, face_states(W0, 0.0)), (1, states_near(rng, W1, 60, 0.5, reach=1.2))])
    return scene("obs_0_1", [W0, W1], st, wo, [plan(0, A, B), plan(1, A, B, t=0.5)], expect=dict(n_obs=[0, 1]))


def uneven_batch(seed):
    """one batch over worlds of 0, 300, 3 and 40 obstacles, with hyperplane and segment counts as uneven; the states and the
    plans name their worlds in no order"""
    rng = np.random.default_rng(seed)
    W0 = p3.PolyWorld3D(*STD_BOX)
    W1 = _crowd(rng, 300, start_t=0.5)
    W2 = p3.PolyWorld3D(*STD_BOX, start_t=1.0)
    W2.static.append(p3.StaticObstacle3D(icosahedron(0.6), (2.8, 0.2, 2.0)))
    W2.linear.append(p3.LinearObstacle3D(p3.box(0.4), (3.5, -1.0, 2.2), (0.0, 0.4, 0.0)))
    W2.nonlinear.append(p3.NonlinearObstacle3D(octahedron(0.7), p3.acc_segs((3.0, 1.5, 1.5), (0.0, -0.4, 0.1), U27[rng.integers(0, 27, 12)] * 0.4, 0.25), start_t=0.3))
    W3 = scatter(rng, p3.PolyWorld3D(*STD_BOX), 20, 5, 15, 0.5, size=(0.2, 0.35), clear=CLEAR, n_seg=(1, 4), line=(A, B))
    worlds = [W0, W1, W2, W3]
    st, wo = _mix([(0, states_in(rng, W0, 20, 0.5)), (1, _std_states(rng, W1, 50, 10, reach=0.5)), (2, states_near(rng, W2, 50, 0.5, reach=1.1)),
                   (3, _std_states(rng, W3, 50, 10))], shuffle=rng)
    plans = [plan(3, A, B, max_expand=150), plan(1, A, B, t=0.5, max_expand=150), plan(0, A, B, max_expand=150), plan(2, A, B, t=1.0, max_expand=150)]
    return scene("uneven_batch", worlds, st, wo, plans, expect=dict(n_obs=[0, 300, 3, 40], unsorted=True))


# ---------------------------------------------------------------- the number of inputs
def _nu_scene(name, seed, U, n_obs, v=(0.0, 0.0, 0.0), goal=B, tags=(), **kw):
    rng = np.random.default_rng(seed)
    W = scatter(rng, p3.PolyWorld3D(*STD_BOX), n_obs // 3, n_obs // 3, n_obs - 2 * (n_obs // 3), 0.5, clear=CLEAR, line=(A, goal))
    st, wo = _mix([(0, np.concatenate([_std_states(rng, W, 120, 50), face_states(W, 0.0)]))])
    return scene(name, [W], st, wo, [plan(0, A, goal, v=v, **kw), plan(0, A + (0.0, 1.0, 0.0), goal + (0.0, 1.0, 0.0), v=v, **kw)], U=U, tags=tags,
                 expect=dict(n_obs=[n_obs], n_u=len(U), pairs=[len(U) * n_obs]))


def nu_1(seed):
    """one input (zero: the robot coasts)"""
    return _nu_scene("nu_1", seed, np.zeros((1, 3)), 9, v=(1.0, 0.0, 0.0), goal=A + (3.0, 0.0, 0.0))


def nu_7(seed):
    """the six-neighbour lattice plus zero"""
    return _nu_scene("nu_7", seed, U7, 12, tags=("jrk",))


def nu_32(seed):
    """a full 32 inputs (POLY3_MAX_U), off the lattice, x 9 obstacles = 288 pairs"""
    rng = np.random.default_rng(seed + 1000)
    U = np.concatenate([np.zeros((1, 3)), U7[1:] * 0.9, np.round(rng.uniform(-1.0, 1.0, (25, 3)), 2)])
    return _nu_scene("nu_32", seed, U, 9, max_expand=300)


# ---------------------------------------------------------------- the box
def box_far(seed):
    """origin (-103.7, 41.3, 12.5), dim (7.3, 11.1, 2.9), world start time 1.25; states on all six faces"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D((-103.7, 41.3, 12.5), (7.3, 11.1, 2.9), start_t=1.25)
    a = W.ori + np.array([1.0, 5.5, 1.5])
    b = a + (3.5, 0.5, 0.0)
    scatter(rng, W, 4, 4, 4, 0.5, clear=[(a, 0.8), (b, 0.8)], line=(a, b))
    st, wo = _mix([(0, np.concatenate([_std_states(rng, W, 110, 40), face_states(W, 1.25), face_states(W, 1.75)]))])
    plans = [plan(0, a, b, t=1.25), plan(0, a, b + (0.0, 1.0, 0.5), t=1.75)]
    return scene("box_far", [W], st, wo, plans, tags=("jrk", "velsnp", "heur"), expect=dict(ori=(-103.7, 41.3, 12.5), dim=(7.3, 11.1, 2.9), start_t=1.25, faces=6))


def box_thin(seed):
    """dim.z = 0.12, less than one primitive's reach along z (u_z = +-1 moves a node at rest 0.125, more than the height):
    most successors leave the box"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D((0.0, -5.0, 1.0), (10.0, 10.0, 0.12))
    a, b = np.array([1.0, 0.0, 1.06]), np.array([4.5, 0.5, 1.06])
    flat = lambda: p3.box(float(rng.uniform(0.25, 0.45)), float(rng.uniform(0.25, 0.45)), 0.3)
    scatter(rng, W, 4, 4, 4, 0.5, clear=[(a, 0.8), (b, 0.8)], poly=flat, line=(a, b))
    for o in W.linear:
        o.v[2] = 0.0
    s = _std_states(rng, W, 140, 60)
    s[:, 5] = rng.choice([0.0, 0.0, 0.1, -0.1], len(s))
    st, wo = _mix([(0, s)])
    return scene("box_thin", [W], st, wo, [plan(0, a, b), plan(0, a, b + (0.0, -1.5, 0.0))], expect=dict(dim_z=0.12, leave_share=0.5))


# ---------------------------------------------------------------- time
def _time_scene(name, seed, dt, start_t, tags=(), plan_t=None, goal=B, v_max=2.0, **kw):
    rng = np.random.default_rng(seed)
    W = scatter(rng, p3.PolyWorld3D(*STD_BOX, start_t=start_t), 4, 4, 4, dt, clear=CLEAR, line=(A, goal))
    below = states_in(rng, W, 20, dt, t0=start_t - 3 * dt)   # node times below the world's start time (and around it)
    off = states_near(rng, W, 20, dt, reach=0.9)
    off[:, 12] += 0.013                                       # off the time lattice
    st, wo = _mix([(0, np.concatenate([_std_states(rng, W, 100, 40, dt=dt), below, off]))])
    t = start_t if plan_t is None else plan_t
    plans = [plan(0, A, goal, t=t, **kw), plan(0, A + (0.0, -1.0, 0.0), goal + (0.0, -1.0, 0.5), t=t + dt, **kw)]
    return scene(name, [W], st, wo, plans, dt=dt, v_max=v_max, tags=tags, expect=dict(dt=dt, start_t=start_t))


def time_dt025(seed):
    """dt 0.25: every other node time is a tie of the key round(t / 0.1) (0.25 / 0.1 = 2.5); world start time 0.37"""
    return _time_scene("time_dt025", seed, 0.25, 0.37, goal=A + (1.2, 0.3, 0.0), plan_t=0.0, eps=3.0, max_expand=600, tags=("jrk",))


def time_dt03(seed):
    """dt 0.3: node times that are no multiple of 0.1 in floating point; world start time 1e3, the plans start at t = 0"""
    return _time_scene("time_dt03", seed, 0.3, 1e3, goal=A + (2.0, 0.3, 0.0), plan_t=0.0, eps=2.0, max_expand=600)


def time_dt1(seed):
    """dt 1.0, world start time -2.0, the plans start at t = 0"""
    return _time_scene("time_dt1", seed, 1.0, -2.0, plan_t=0.0, tags=("heur",), goal=A + (5.0, 0.5, 0.0))


def deep(seed):
    """dt 0.1, v_max 1, eps 5 over 4.6 m of a lightly obstructed world: the deepest expanded node is 40 or more levels down"""
    rng = np.random.default_rng(seed)
    W = scatter(rng, p3.PolyWorld3D(*STD_BOX), 3, 3, 3, 0.5, clear=[(A, 0.8), (A + (4.6, 0.0, 0.0), 0.8)])
    W.static.append(p3.StaticObstacle3D(p3.box(0.3), A + (2.3, -0.5, 0.0)))  # beside the straight line
    near = states_near(rng, W, 120, 0.1, v=0.9, reach=0.5, levels=60)
    st, wo = _mix([(0, np.concatenate([near, states_in(rng, W, 40, 0.1, v=0.9, levels=60)]))])
    plans = [plan(0, A, A + (4.6, 0.0, 0.0), v=(1.0, 0.0, 0.0), eps=5.0, max_expand=600), plan(0, A + (0.0, 1.5, 0.0), A + (2.0, 1.5, 0.5), eps=5.0, max_expand=600)]
    return scene("deep", [W], st, wo, plans, U=U7, dt=0.1, v_max=1.0, expect=dict(min_levels=40))


# ---------------------------------------------------------------- the degree of the obstacle trajectories
def _high_segs(rng, p0, v0, n, dt, kind):
    """n chained segments of duration dt from (p0, v0).  kind "z3": ACC on x and y, a jerk on z only; "45": quartic and quintic
    segments in turn on every axis (coefficients c0 t^5 / 120 + c1 t^4 / 24 + c2 t^3 / 6 + c3 t^2 / 2 + c4 t + c5)"""
    rows, p, v = [], np.array(p0, float), np.array(v0, float)
    for k in range(n):
        c = np.zeros((3, 6))
        c[:, 3] = np.round(rng.uniform(-0.6, 0.6, 3), 1)
        if kind == "z3":
            c[2, 2] = float(rng.choice([-1.5, -1.0, 1.0, 1.5]))
        elif k % 2:
            c[:, 1] = np.round(rng.uniform(-6.0, 6.0, 3), 0)
        else:
            c[:, 0] = np.round(rng.uniform(-40.0, 40.0, 3), 0)
            c[0, 1] = 3.0
        c[:, 4], c[:, 5] = v, p
        rows.append(list(c.reshape(-1)) + [dt])
        t = dt
        p = c[:, 0] / 120 * t ** 5 + c[:, 1] / 24 * t ** 4 + c[:, 2] / 6 * t ** 3 + c[:, 3] / 2 * t * t + c[:, 4] * t + c[:, 5]
        v = np.round(c[:, 0] / 24 * t ** 4 + c[:, 1] / 6 * t ** 3 + c[:, 2] / 2 * t * t + c[:, 3] * t + c[:, 4], 3)
    return np.array(rows).reshape(-1, 19)


def _degree_scene(name, seed, kind, tags, n_worlds=1):
    rng = np.random.default_rng(seed)
    worlds = []
    for k in range(n_worlds):
        W = p3.PolyWorld3D(*STD_BOX, start_t=0.5 * k)
        scatter(rng, W, 1, 1, 8, 0.5, size=(0.4, 0.6), clear=CLEAR, speed=0.3, cov=(0.0,), line=(A, B),
                segs=lambda p0, v0: _high_segs(rng, p0, v0, int(rng.integers(4, 9)), 0.5, kind))
        for o in W.nonlinear:
            o.start_t, o.disappear_front, o.disappear_back = float(rng.choice([0.0, 0.3])), False, False
        worlds.append(W)
    st, wo = _mix([(k, np.concatenate([states_near(rng, W, 100 // n_worlds, 0.5, reach=0.9, only=W.nonlinear), states_in(rng, W, 30 // n_worlds, 0.5)]))
                   for k, W in enumerate(worlds)])
    plans = [plan(k % n_worlds, A, B + (0.0, 0.5 * (k // n_worlds), 0.0), t=0.5 * (k % n_worlds), max_expand=120) for k in range(3)]
    return scene(name, worlds, st, wo, plans, tags=tags, expect=dict(gen_acc=True, degree=kind))


def degree_z3(seed):
    """obstacle trajectories cubic on the z axis only: ACC primitives take the general solver"""
    return _degree_scene("degree_z3", seed, "z3", ("velsnp",))


def degree_4_5(seed):
    """quartic and quintic segments, two worlds"""
    return _degree_scene("degree_4_5", seed, "45", ("jrk",), n_worlds=2)


def jerk_zero(seed):
    """obstacle segments built as JRK primitives whose jerk is exactly zero (and -0.0): they count as quadratic"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D(*STD_BOX)

    def segs(p0, v0):
        sg = p3.jrk_segs(p0, v0, np.round(rng.uniform(-0.5, 0.5, 3), 1), np.zeros((int(rng.integers(3, 7)), 3)), 0.5)
        sg[::2, [2, 8, 14]] = -0.0
        return sg
    scatter(rng, W, 2, 2, 8, 0.5, size=(0.35, 0.55), clear=CLEAR, segs=segs, line=(A, B))
    st, wo = _mix([(0, _std_states(rng, W, 120, 40))])
    return scene("jerk_zero", [W], st, wo, [plan(0, A, B), plan(0, A, B + (0.0, -1.0, -0.5))], tags=("jrk",), expect=dict(gen_acc=False, jrk_built=True))


def seg_short(seed):
    """trajectories of 30 segments of dt / 10 (a primitive spans six of them and more), one zero-duration segment among them"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D(*STD_BOX)
    for k in range(8):
        sg = p3.acc_segs((2.5 + 0.9 * k, -1.5 + 3.0 * (k % 2), 1.5 + 0.3 * (k % 3)), np.round(rng.uniform(-0.4, 0.4, 3), 1), U27[rng.integers(0, 27, 30)] * 0.6, 0.05)
        if k % 2 == 0:  # a zero-duration segment in the middle (never selected)
            z = sg[7].copy()
            z[18] = 0.0
            sg = np.concatenate([sg[:7], z[None], sg[7:]])
        W.nonlinear.append(p3.NonlinearObstacle3D(octahedron(0.8) if k % 2 else p3.box(0.5), sg, start_t=0.0 if k < 4 else 0.3, disappear_back=bool(k % 4 == 1)))
    W.static.append(p3.StaticObstacle3D(p3.box(0.4), (3.0, 0.3, 2.0)))
    st, wo = _mix([(0, _std_states(rng, W, 90, 30, reach=0.9))])
    st[:, 12] = np.where(np.arange(len(st)) % 3 == 0, st[:, 12] % 1.5, st[:, 12])
    return scene("seg_short", [W], st, wo, [plan(0, A, B), plan(0, A + (0.0, 1.0, 0.0), B + (0.5, 1.0, 0.0))], tags=("jrk", "velsnp"),
                 expect=dict(overlaps={10, 11}, n_seg={30, 31}, zero_T=4))


def presence(seed):
    """disappear_front / disappear_back in the four combinations; node times before, at 0, inside, at total_t and after the trajectory"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D(*STD_BOX)
    for k, (front, back) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        sg = p3.acc_segs((2.0 + 2.0 * k, -2.0, 2.0), (0.0, 1.0, 0.0), np.zeros((3, 3)), 0.5)  # 1.5 s straight along y from -2 to -0.5
        W.nonlinear.append(p3.NonlinearObstacle3D(p3.box(0.5), sg, start_t=-1.0, disappear_front=front, disappear_back=back))
    ss = []
    for t in (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5):  # traj_t = t - 1: -1, -0.5, 0 (= start), 0.5, 1, 1.5 (= total_t), 2, 2.5
        for k in range(4):
            for y in (-2.0, -1.2, -0.5, 0.3):  # at the clamped start, on the way, at the clamped end, just beyond
                ss.append([2.0 + 2.0 * k + 0.7, y, 2.0 + 0.2 * (k % 2), -0.6, 0.0, 0.0, 0, 0, 0, 0, 0, 0, t])
    st, wo = _mix([(0, np.array(ss)), (0, states_in(rng, W, 40, 0.5))])
    plans = [plan(0, (0.5, -1.2, 2.0), (4.0, -1.2, 2.0)), plan(0, (0.5, -1.2, 2.0), (4.0, -1.2, 2.0), t=2.0)]
    return scene("presence", [W], st, wo, plans, tags=("velsnp",), expect=dict(traj_times={-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5}, total_t=1.5))


def overrun(seed):
    """obstacles that come over lattice nodes while a plan is in flight: a linear one sweeping across the straight line, nonlinear
    ones that sweep and -- disappear_front -- stand on nodes of the line from t = 1.0 / 1.5 on without having been anywhere
    before: a node reached at that very time was reached by a free primitive, and its own start-point test fails"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D(*STD_BOX)
    W.linear.append(p3.LinearObstacle3D(p3.box(0.4), (3.0, -2.0, 2.0), (0.0, 1.0, 0.0)))
    for x, t0, hy in ((1.375, 1.0, 0.45), (2.0, 1.5, 0.3), (1.5, 1.5, 0.3)):
        sg = p3.acc_segs((x, 0.0, 2.0), (0.0, 0.0, 0.0), np.zeros((2, 3)), 0.5)   # standing for 1 s, from its appearance at t0 on
        W.nonlinear.append(p3.NonlinearObstacle3D(p3.box(0.2, hy, 0.3), sg, start_t=-t0, disappear_front=True, disappear_back=True))
    W.nonlinear.append(p3.NonlinearObstacle3D(octahedron(0.7), p3.acc_segs((4.0, 2.5, 2.0), (0.0, -1.0, 0.0), U27[[13, 13, 4, 13, 22, 13]] * 0.5, 0.5), start_t=0.0))
    st, wo = _mix([(0, _std_states(rng, W, 120, 40, reach=0.8))])
    plans = [plan(0, A, B), plan(0, A, B, t=0.5), plan(0, A + (0.0, -0.5, 0.0), B)]
    return scene("overrun", [W], st, wo, plans, tags=("jrk",), expect=dict(start_hit_mid_plan=True))


def shapes(seed):
    """one half-space, a slab, a 20-face tilted polyhedron, a reference point outside its shape; linear obstacles with cov_v > 0
    and with zero velocity"""
    rng = np.random.default_rng(seed)
    W = p3.PolyWorld3D(*STD_BOX)
    W.static.append(p3.StaticObstacle3D(half_space((-0.1, -0.2, -1.0), 0.0), (5.0, 0.0, 3.4)))         # all that lies above a tilted plane near z = 3.4
    W.linear.append(p3.LinearObstacle3D(slab((1.0, 0.3, 0.2), 0.15), (7.5, 0.0, 2.0), (-0.2, 0.0, 0.0)))  # a thin unbounded wall drifting towards -x
    W.nonlinear.append(p3.NonlinearObstacle3D(icosahedron(0.6), p3.acc_segs((3.0, -1.5, 1.5), (0.2, 0.1, 0.1), U27[[5, 3, 8, 0]] * 0.5, 0.5), start_t=0.0))
    W.static.append(p3.StaticObstacle3D(icosahedron(0.5, center=(2.0, 1.5, 0.5)), (1.0, -0.5, 1.5)))  # reference point 2.5 away from the shape at (3, 1, 2)
    W.linear.append(p3.LinearObstacle3D(octahedron(0.6), (6.0, 2.0, 2.0), (0.0, 0.0, 0.0), cov_v=0.1))  # standing and growing
    W.linear.append(p3.LinearObstacle3D(p3.box(0.4), (4.0, -2.5, 2.5), (0.0, 0.0, 0.0)))               # standing
    W.linear.append(p3.LinearObstacle3D(icosahedron(0.4), (8.0, -3.0, 1.0), (-0.5, 0.4, 0.2), cov_v=0.1))
    near = states_near(rng, W, 110, 0.5, reach=1.0, only=[o for o in obstacles(W) if len(o.poly) > 2] + [W.static[1]])
    near[:30, 0:3] = np.round((3.0, 1.0, 2.0) + rng.uniform(-1.0, 1.0, (30, 3)), 2)  # around the shape that is away from its reference point
    top = states_in(rng, W, 30, 0.5)
    top[:, 2] = np.round(rng.uniform(3.0, 3.9, 30), 2)
    st, wo = _mix([(0, np.concatenate([near, top, states_in(rng, W, 30, 0.5)]))])
    plans = [plan(0, A, (4.0, 1.5, 2.0)), plan(0, A, B + (1.0, -1.0, 0.5), gv=(0.5, 0.0, 0.0))]
    return scene("shapes", [W], st, wo, plans, tags=("velsnp", "tolvel"), expect=dict(n_hp={1, 2, 6, 8, 20}, outside_ref=True, cov_pos=2, v_zero=2))


def limits_off(seed):
    """v_max = a_max = j_max = -1: validate_primitive passes everything"""
    rng = np.random.default_rng(seed)
    W = scatter(rng, p3.PolyWorld3D(*STD_BOX), 4, 4, 4, 0.5, clear=CLEAR, line=(A, B))
    s = _std_states(rng, W, 110, 40)
    s[:, 3:6] *= 3.0
    st, wo = _mix([(0, s)])
    return scene("limits_off", [W], st, wo, [plan(0, A, B, max_expand=600), plan(0, A, A + (2.0, 1.0, 0.5), max_expand=600)], v_max=-1.0, a_max=-1.0, j_max=-1.0,
                 tags=("jrk",), expect=dict(limits=False))


SCENES = {f.__name__: f for f in (pairs_one_pass, pairs_strided, obs_300, obs_0_1, uneven_batch, nu_1, nu_7, nu_32, box_far, box_thin, time_dt025, time_dt03,
                                  time_dt1, deep, degree_z3, degree_4_5, jerk_zero, seg_short, presence, overrun, shapes, limits_off)}
SEED = 3024
JRK_REACH, JRK_CAP = 1.5, 300
_made = {}


def get(name):
    """the scene of the fixed seed, built once per process"""
    if name not in _made:
        _made[name] = SCENES[name](SEED + sorted(SCENES).index(name))
        assert _made[name].name == name
    return _made[name]


def with_control(S, control, U=None, **env):
    """the scene under another control kind (and, if given, another lattice / set-up): same worlds, the states given the
    acceleration (JRK, SNP) and jerk (SNP) the kind carries, seeded per scene.  A JRK state space grows much faster (27 inputs,
    nine key integers and the time): the plans start with a velocity towards their goal, the goal is brought to JRK_REACH of the
    start and the cap to JRK_CAP, so that plans are found within what the CPU checker runs in a second or two."""
    rng = np.random.default_rng(SEED + 7 * control + sorted(SCENES).index(S.name))
    st = S.states.copy()
    if control in (JRK, SNP):
        st[:, 6:9] = np.round(rng.uniform(-0.8, 0.8, (len(st), 3)), 1)
    if control == SNP:
        st[:, 9:12] = np.round(rng.uniform(-1, 1, (len(st), 3)), 1)
    dt = env.get("dt", S.dt)
    if dt != S.dt:
        st[:, 12] = np.round((st[:, 12] - S.worlds[0].start_t) / S.dt) * dt + S.worlds[0].start_t
    plans = []
    for p in S.plans:
        d = p["goal"][0:3] - p["start"][0:3]
        n = float(np.linalg.norm(d))
        s, g = p["start"].copy(), p["goal"].copy()
        g[0:3] = s[0:3] + d * min(1.0, JRK_REACH / n)
        if not np.any(s[3:6]):
            s[3:6] = np.round(0.5 * d / n, 1)
        plans.append(dict(world=p["world"], start=s, goal=g, kw=dict(p["kw"], max_expand=JRK_CAP)))
    return Scene(S.name, S.worlds, st, S.world_of, plans, control=control, U=S.U if U is None else U, tags=S.tags, expect=S.expect, **dict(S.env, **env))
