"""Seeded point clouds for the point-cloud planner's tests: an "office-shaped" scene that matches
mpl_test_node/launch/ellipsoid_planner_node/test.launch (box origin (6, 12, 0), range (25, 5, 1.5), start (8, 13, 1.3),
goal (28.5, 14, 1.3)) -- outer walls, partition walls with doorways, pillars and desks as points on a 0.05 m lattice,
every coordinate a float32 value, plus a handful of points outside the box -- and the launch file's parameters."""
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
