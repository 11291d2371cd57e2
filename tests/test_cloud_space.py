"""The device-side state-space export of the point-cloud planner (include/mplx_space.h: mplx_cloud_result_space_counts / _space /
_space_edges; EllipsoidPlanner.state_space / state_spaces) against the CPU checkers (tests/cloud_checker.py, tests/cloud_prior_checker.py)
on the door scene: states, g, h, flags and predecessor lists in arrival order, single queries and the slot-reuse batch.
Everything compared is a moved f64 or an integer: every comparison is exact."""
import numpy as np
import pytest

from oracle import orc
from tests import cloud_checker as K
from tests import cloud_prior_checker as PC
from tests import cloud_scenes as S
from tests import test_cloud_geometry as G
from tests import test_cloud_prior as TP

pytestmark = pytest.mark.gpu

KEYS = ("states", "g", "h", "closed", "opened", "child", "parent", "action")
_ref = {}


class Recording:
    """mixin of a checker (cloud_checker.Checker or cloud_prior_checker.Checker): plan() also returns what the checker's plan() keeps in
    locals, recorded WHILE it is built and not computed a second time --
      h      the value of every heuristic call the checker's `create` makes, in creation order (cloud_checker.py: h.append(0.0 if eps
             == 0 else P.heuristic(w)); cloud_prior_checker returns its own `h` and is left alone);
      preds  the checker appends (cur, a, cost) to the list of the successor's state for every valid record get_succ returns, expansion
             by expansion: the records get_succ handed out are kept per call, and filed under the state their key names."""

    def get_succ(self, s13):
        out = super().get_succ(s13)
        if self._calls is not None:
            self._calls.append(out)
        return out

    _calls = None

    def plan(self, start, goal, **kw):
        heur, values = orc.Planner.heuristic, []

        def recording(planner, state):
            v = heur(planner, state)
            values.append(v)
            return v

        self._calls = []
        orc.Planner.heuristic = recording
        try:
            res = super().plan(start, goal, **kw)
        finally:
            orc.Planner.heuristic = heur
            calls, self._calls = self._calls, None
        if not res["states"]:  # (the start satisfied the goal: nothing was created)
            res.update(g=[], h=[], closed=[], opened=[], preds=[])
            return res
        if "h" not in res:
            res["h"] = values if values else [0.0] * len(res["states"])  # (eps 0: no heuristic call, h = 0)
            assert len(res["h"]) == len(res["states"])
        assert len(calls) == len(res["expanded"])  # one get_succ per expansion
        table = {K.key_of(K.state_wp(s, self.control)): i for i, s in enumerate(res["states"])}
        preds = [[] for _ in res["states"]]
        for cur, out in zip(res["expanded"], calls):
            for ok, st, cost, a in out:
                if ok:
                    preds[table[K.key_of(K.state_wp(st * self.mask, self.control))]].append((cur, a))
        res["preds"] = preds
        return res


class SpaceChecker(Recording, G.PlanChecker):
    """the door checker whose plan() also returns `h` and `preds`"""


class PriorSpaceChecker(Recording, PC.Checker):
    """the prior checker whose plan() also returns `preds` (`h` is its own)"""


def door_checker(control, hid=False):
    sc = S.SCENES[G.DOOR]
    ck = S.checker(sc, control, S.build(G.DOOR, control)[0], cls=SpaceChecker)
    ck.extra = dict(heur_ignore_dynamics=hid)
    return ck


def compare(ss, c):
    """an exported state space against a checker result"""
    n = len(c["states"])
    assert ss["states"].shape == (n, 13) and np.array_equal(ss["states"], np.array(c["states"], dtype=np.float64).reshape(n, 13))
    assert np.array_equal(ss["g"], np.array(c["g"], dtype=np.float64)) and np.array_equal(ss["h"], np.array(c["h"], dtype=np.float64))
    assert ss["closed"].tolist() == [int(x) for x in c["closed"]] and ss["opened"].tolist() == [int(x) for x in c["opened"]]
    rec = [(i, p, a) for i, lst in enumerate(c["preds"]) for p, a in lst]
    assert list(zip(ss["child"].tolist(), ss["parent"].tolist(), ss["action"].tolist())) == rec


def same(a, b, keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 6. single plans
@pytest.mark.parametrize("control", [orc.VEL, orc.ACC, orc.SNP], ids=["VEL", "ACC", "SNP"])
def test_easy_pair_equals_the_checker(control):
    start, goal = G.door_query(S.SCENES[G.DOOR]["pairs"]["easy"])
    c = G.checker_plan(door_checker(control), start, goal, 400)
    pl = G.door_device(control, False)
    pl.set_max_num(400)
    pl.plan(start, goal)
    r = pl.result()
    assert r["status"] == c["status"] and r["n_nodes"] == len(c["states"]) > 9
    ss = pl.state_space(0)
    assert len(ss["child"]) == r["n_edges"] >= r["n_nodes"] - 1
    compare(ss, c)
    st, g, cl, op = pl.nodes(0)  # the host-decoded getter
    assert np.array_equal(ss["states"], st) and np.array_equal(ss["g"], g)
    assert np.array_equal(ss["closed"] == 1, cl) and np.array_equal(ss["opened"] == 1, op)
    nk = {orc.VEL: 3, orc.ACC: 6, orc.SNP: 12}[control]
    assert np.all(ss["states"][:, nk:12] == 0.0) and np.any(ss["states"][:, nk - 3:nk] != 0.0)
    assert np.any(ss["h"] != 0.0)


def test_guided_plan_equals_the_prior_checker():
    control, start, goal, _, eps = TP.PLAN_CASES["short"]
    prior = TP.reference("short")[0]
    from mpl_ros_amd.ellipsoid import control_lattice
    ck = PriorSpaceChecker(K.Cloud(TP.room(), TP.R, TP.ORI, TP.DIM), control, control_lattice(TP.U_OF[control], 1, False), TP.DT, v_max=TP.V_MAX,
                           a_max=TP.A_MAX, w=TP.W)
    c = ck.plan(start, goal, prior=prior, eps=eps, **TP.KW)
    pl = TP.device(control)
    pl.set_epsilon(eps)
    pl.set_prior_trajectory(prior)
    pl.plan(start, goal)
    assert pl.result()["status"] == c["status"]
    compare(pl.state_space(0), c)


# ------------------------------------------------------------------------------------------------ 7. the slot-reuse batch
def reuse_reference():
    if "reuse" not in _ref:
        ck = door_checker(orc.VEL, True)
        _ref["reuse"] = {q: G.checker_plan(ck, *G.door_query(S.REUSE_QUERIES[q]), S.REUSE_MAX_NUM) for q in range(0, 16, 4)}
    return _ref["reuse"]


def test_sixteen_queries_on_three_slots_many_form_equals_singles_and_checker():
    starts, goals = [np.array(x) for x in zip(*[G.door_query(q) for q in S.REUSE_QUERIES])]
    pl = G.door_device(orc.VEL, True, slots=3)
    pl.set_max_num(S.REUSE_MAX_NUM)
    batch = pl.plan_batch(starts, goals)
    assert {(b["status"], b["n_expanded"] > 0) for b in batch} == {(0, True), (0, False), (1, True), (3, True)}
    many = pl.state_spaces()
    singles = [pl.state_space(q) for q in range(16)]
    assert many["node_off"].tolist() == np.concatenate([[0], np.cumsum([b["n_nodes"] for b in batch])]).tolist()
    assert many["edge_off"].tolist() == np.concatenate([[0], np.cumsum([b["n_edges"] if b["n_nodes"] else 0 for b in batch])]).tolist()
    assert any(b["n_nodes"] == 0 for b in batch[1:15])  # (start-is-goal queries in the middle: no rows)
    for k in KEYS:
        assert np.array_equal(many[k], np.concatenate([s[k] for s in singles])), k
    order = [15, 3, 0, 7, 12, 8]
    lst = pl.state_spaces(order)
    for k in KEYS:
        assert np.array_equal(lst[k], np.concatenate([singles[q][k] for q in order])), k
    for q, c in reuse_reference().items():
        assert batch[q]["status"] == c["status"]
        compare(singles[q], c)
    # a query planned alone leaves the same state space
    one_pl = G.door_device(orc.VEL, True)
    one_pl.set_max_num(S.REUSE_MAX_NUM)
    for q in (1, 2, 3):
        one_pl.plan_batch(starts[q:q + 1], goals[q:q + 1])
        same(one_pl.state_space(0), singles[q])


def test_refusals_carry_the_clouds_error_text():
    from mpl_ros_amd import _capi
    from mpl_ros_amd._capi import MplxError
    start, goal = G.door_query(S.SCENES[G.DOOR]["pairs"]["easy"])
    pl = G.door_device(orc.VEL, True)
    pl.set_max_num(50)
    lib = pl.lib
    sent = np.full((8, 13), -7.25)
    q = np.array([0], dtype=np.int32)
    assert lib.mplx_cloud_result_space(pl.h, 1, q.ctypes.data, 8, sent.ctypes.data, None, None, None, None) == _capi.ERR_ARG
    assert b"no batch" in lib.mplx_cloud_last_error(pl.h) and np.all(sent == -7.25)
    assert lib.mplx_cloud_result_space(None, 1, None, 8, sent.ctypes.data, None, None, None, None) == _capi.ERR_ARG
    pl.plan(start, goal)
    n = pl.result()["n_nodes"]
    assert n > 8
    assert lib.mplx_cloud_result_space(pl.h, 1, q.ctypes.data, 8, sent.ctypes.data, None, None, None, None) == _capi.ERR_CAPACITY and np.all(sent == -7.25)
    with pytest.raises(MplxError, match="no query 1"):
        pl.state_space(1)
    with pytest.raises(MplxError, match="twice"):
        pl.state_spaces([0, 0])
    assert len(pl.state_space(0)["g"]) == n
