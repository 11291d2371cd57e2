#!/usr/bin/env python3
"""Writes tests/golden/lpa_fleet_pairs.json: the start / goal pairs of the LPA* fleet scenarios F2 and F3 (tests/test_lpa_fleet.py).
The pairs are drawn with numpy's default_rng(20261016) and kept as a fixture so that a numpy version cannot move them; the CPU
checker (oracle/) decides which draws are connected.  usage: tools/make_lpa_fleet_pairs.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpl_ros_amd import mapgen  # noqa: E402
from oracle import orc  # noqa: E402
from tests import test_lpa as T  # noqa: E402
from tests import util  # noqa: E402

SEED = 20261016


def pairs_f2(n=16):
    """2-D lattice on simple_map.npz: one end in the left part of the map, the other in the right part"""
    sc = T.Scenario()
    free2d = sc.grid[0] == 0
    rng = np.random.default_rng(SEED)
    pairs, draws = [], 0
    while len(pairs) < n:
        draws += 1
        s = np.array([rng.integers(5, 60), rng.integers(5, 174)])
        g = np.array([rng.integers(120, 174), rng.integers(5, 174)])
        if rng.integers(0, 2):
            s, g = g, s
        if not (free2d[s[1], s[0]] and free2d[g[1], g[0]]):
            continue
        ps = ((s[0] + 0.5) * 0.1, (s[1] + 0.5) * 0.1, 0.025)
        pg = ((g[0] + 0.5) * 0.1, (g[1] + 0.5) * 0.1, 0.025)
        if sc.scratch.plan(orc.waypoint(ps), orc.waypoint(pg)) != orc.OK:
            continue
        pairs.append([[float(v) for v in ps], [float(v) for v in pg]])
    return pairs, draws


def pairs_f3(n=8):
    """27 inputs on skir_map.npz: both ends uniform over the grid's cells, free, at least 4 m apart, connected"""
    grid, origin, res, _, _, _ = T.scenario_3d("skir")
    U = mapgen.control_lattice(1.0, 1, True)
    probe = util.make_oracle(grid, origin, res, orc.ACC, U, **T.KW3)
    dz, dy, dx = grid.shape
    rng = np.random.default_rng(SEED)
    pairs, draws = [], 0
    while len(pairs) < n:
        draws += 1
        s = rng.integers(0, [dx, dy, dz])
        g = rng.integers(0, [dx, dy, dz])
        if grid[s[2], s[1], s[0]] != 0 or grid[g[2], g[1], g[0]] != 0:
            continue
        ps = tuple(float(origin[k] + (s[k] + 0.5) * res) for k in range(3))
        pg = tuple(float(origin[k] + (g[k] + 0.5) * res) for k in range(3))
        if np.linalg.norm(np.array(ps) - np.array(pg)) < 4.0:
            continue
        if probe.plan(orc.waypoint(ps), orc.waypoint(pg)) != orc.OK:
            continue
        pairs.append([list(ps), list(pg)])
    return pairs, draws


if __name__ == "__main__":
    f2, d2 = pairs_f2()
    f3, d3 = pairs_f3()
    out = dict(seed=SEED, F2=f2, F2_draws=d2, F3=f3, F3_draws=d3)
    path = os.path.join(ROOT, "tests", "golden", "lpa_fleet_pairs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{path}: F2 {len(f2)} pairs of {d2} draws, F3 {len(f3)} pairs of {d3} draws")
