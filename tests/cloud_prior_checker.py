"""CPU checker of the point-cloud search guided by a prior trajectory: the A* of tests/cloud_checker.py with the heuristic of
the P-list (mpl_ros_amd/csrc/mplx_cloud.h): P1 sampling, P2 get_heur, P3 the time of the creating arrival, P4 the start's
time, P5 everything else unchanged.  get_succ, the keys and the goal test are cloud_checker's; cal_heur towards an arbitrary
target is the oracle's (orc.Planner.set_goal + heuristic on a planner of its own per prior entry).  Test infrastructure only.
"""
import ctypes as C
import heapq
import math

import numpy as np

from oracle import orc
from tests import cloud_checker as CC


def sample_prior(evaluate, T, dt, w, control):
    """P1: for (t = 0; t < T; t += dt) {evaluate(t), w (T - t)}; evaluate(t) returns 12 doubles (pos vel acc jrk)"""
    st, ctg = [], []
    t = 0.0
    while t < T:
        st.append(list(evaluate(t)) + [t])
        ctg.append(w * (T - t))
        t += dt
    n = len(ctg)
    return {"states": np.array(st, dtype=np.float64).reshape(n, 13), "controls": np.full(n, control & 15, dtype=np.int32),
            "cost_to_go": np.array(ctg, dtype=np.float64)}


class PriorHeuristic:
    """P2 for one goal and one prior table"""

    def __init__(self, control, U, dt, v_max, w, goal13, prior=None, heur_ignore_dynamics=False, **cfg):
        self.control, self.dt = control, float(dt)
        self.kw = dict(dt=dt, v_max=v_max, w=w, heur_ignore_dynamics=heur_ignore_dynamics, **cfg)
        self.U = U
        self.P = self._planner(CC.state_wp(goal13, control))
        self.goal_key = CC.key_of(CC.state_wp(goal13, control))
        self.prior = prior
        self.n = 0 if prior is None else len(prior["cost_to_go"])
        self.targets = {}

    def _planner(self, target):
        P = orc.Planner()
        P.set_config(self.control, self.U, **self.kw)
        P.set_goal(target)
        return P

    def _target(self, i):
        """a planner whose goal is prior entry i.  The entry's waypoint carries the yaw bit on top of its control kind: the
        oracle's heuristic then never takes its "same key as the goal: 0" shortcut (the controls differ) while cal_heur
        itself looks at the low four bits only -- what remains is cal_heur(state -> entry), as P2 asks."""
        if i not in self.targets:
            s = [float(x) for x in self.prior["states"][i]]
            k = int(self.prior["controls"][i]) & 15
            self.targets[i] = self._planner(orc.waypoint(s[0:3], s[3:6], s[6:9], s[9:12], control=k | orc.YAW, t=s[12]))
        return self.targets[i]

    def __call__(self, s13):
        w = CC.state_wp(s13, self.control)
        if CC.key_of(w) == self.goal_key:
            return 0.0
        t = float(s13[12])
        if self.n > 0 and t >= 0.0:
            x = t / self.dt
            if x < self.n:
                i = int(x)
                return self._target(i).heuristic(w) + float(self.prior["cost_to_go"][i])
        return self.P.heuristic(w)


class Checker(CC.Checker):
    """cloud_checker.Checker whose plan() takes a prior table"""

    def plan(self, start, goal, prior=None, eps=1.0, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, max_num=-1, heur_ignore_dynamics=False):
        P = orc.Planner()
        P.set_config(self.control, self.U, dt=self.dt, v_max=self.v_max, a_max=self.a_max, j_max=self.j_max, w=self.w, eps=eps,
                     tol_pos=tol_pos, tol_vel=tol_vel, tol_acc=tol_acc, max_expand=max_num, heur_ignore_dynamics=heur_ignore_dynamics)
        P.set_goal(CC.state_wp(goal, self.control))
        sw = CC.state_wp(start, self.control)
        res = {"status": 0, "cost": math.inf, "expanded": [], "states": [], "g": [], "closed": [], "traj": None}
        if P.is_goal(sw):
            res["cost"] = 0.0
            return res
        heur = PriorHeuristic(self.control, self.U, self.dt, self.v_max, self.w, np.array(goal, dtype=np.float64) * self.mask, prior,
                              heur_ignore_dynamics=heur_ignore_dynamics, a_max=self.a_max, j_max=self.j_max)
        states, g, h, closed, opened, preds = [], [], [], [], [], []
        table = {}

        def create(s13, w):  # (P3: h from the time of the arrival that creates the state)
            table[CC.key_of(w)] = len(states)
            states.append(s13); g.append(math.inf); closed.append(False); opened.append(False); preds.append([])
            h.append(0.0 if eps == 0 else heur(s13))
            return len(states) - 1

        sid = create(np.array(start, dtype=np.float64) * self.mask, sw)  # (P4)
        g[sid], opened[sid] = 0.0, True
        heap = [(g[sid] + eps * h[sid], 0.0, sid)]
        n_reopen, n_open, it, status = 0, 1, 0, 0
        while True:
            it += 1
            while True:  # pop, dropping stale entries
                f, gg, cur = heapq.heappop(heap)
                if not closed[cur] and gg == g[cur]:
                    break
            closed[cur] = True
            n_open -= 1
            res["expanded"].append(cur)
            for ok, st, cost, a in self.get_succ(states[cur]):
                if not ok:
                    continue
                st = st * self.mask
                w = CC.state_wp(st, self.control)
                sid2 = table.get(CC.key_of(w))
                if sid2 is None:
                    sid2 = create(st, w)
                preds[sid2].append((cur, a, cost))
                tent = g[cur] + cost
                if tent < g[sid2]:
                    if closed[sid2]:
                        n_reopen += 1  # D6
                    if closed[sid2] or not opened[sid2]:
                        n_open += 1
                    g[sid2] = tent
                    closed[sid2] = False
                    opened[sid2] = True
                    heapq.heappush(heap, (tent + eps * h[sid2], tent, sid2))
            if P.is_goal(CC.state_wp(states[cur], self.control)):
                break
            if max_num > 0 and it >= max_num:
                status = 3
                break
            if n_open == 0:
                status = 1
                break
        res.update(status=status, states=states, g=g, h=h, closed=closed, opened=opened, n_reopen=n_reopen)
        if status != 0:
            return res
        node, nodes, acts = cur, [cur], []
        while preds[node]:
            best, mr, mg = None, math.inf, math.inf
            for par, a, c in preds[node]:
                rhs = g[par] + c
                if rhs < mr or (rhs == mr and mg < g[par]):
                    best, mr, mg = (par, a), rhs, g[par]
            node = best[0]
            acts.append(best[1])
            nodes.append(node)
            if node == sid:
                break
        nodes.reverse(), acts.reverse()
        res["cost"] = g[cur]
        res["traj"] = {"node_ids": nodes, "actions": acts, "states": np.array([states[i] for i in nodes])}
        return res
