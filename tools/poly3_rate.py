"""Numbers of the 3-D moving-obstacle planner (no gate): kernel time and expansions per second of batches of 1 / 16 / 64
queries, each query in its own seeded 3-D world (tests/test_poly_map3d.py's random_world3d: static boxes and octahedra, linear
and nonlinear obstacles), ACC control, the 27-input lattice, the dynamics-aware heuristic, capped at 1500 expansions.
usage: python tools/poly3_rate.py [--reps N]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpl_ros_amd import poly_map3d as p3  # noqa: E402
from tests.test_poly_map3d import KW3, random_world3d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    worlds = [random_world3d(rng, jrk_obstacles=False) for _ in range(64)]
    U = p3.control_lattice(1.0, 1)
    team = p3.PolyTeam3D()
    team.configure(p3.ACC, U, **KW3)
    team.set_worlds(worlds)
    team.set_capacity(64, 1 << 22, 1 << 24, 1 << 23)
    starts, goals = np.zeros((64, 13)), np.zeros((64, 13))
    starts[:, 0:3] = np.round(rng.uniform((0.5, -4.5, 0.5), (2.5, 4.5, 3.5), (64, 3)), 1)
    goals[:, 0:3] = starts[:, 0:3] + np.round(rng.uniform((1.5, -1.5, -0.5), (3.0, 1.5, 0.5), (64, 3)), 1)
    out = {}
    for n in (1, 16, 64):
        w = np.arange(n)
        team.plan_batch(w, starts[:n], goals[:n], max_expand=1500, heur_ignore_dynamics=False)  # warm-up
        ms, exp = [], 0
        for _ in range(a.reps):
            R = team.plan_batch(w, starts[:n], goals[:n], max_expand=1500, heur_ignore_dynamics=False)
            ms.append(team.last_kernel_ms())
            exp = sum(int(r.n_expanded) for r in R)
        med = float(np.median(ms))
        out[f"batch_{n}"] = {"kernel_ms_median": med, "expansions": exp, "expansions_per_s": exp / (med * 1e-3),
                             "ok": sum(int(r.status == 0) for r in R)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
