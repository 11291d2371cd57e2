"""The look-up of astar_spec_kernel<32,16,ACC,help> with its first probe step peeled (mplx_spec.h MPLX_X_LOOKUP_OVERLAP):
the claim of an empty slot or the record of an entry is asked for before anything waits, a home slot that is final and not the
query's is passed over from the two slot words the lane holds, and the probe loop takes over from the second or third step.

What can go wrong there: a slot passed over that should have matched (a state created twice: more states, another expansion
order), a claim left unresolved (helpers or a later look-up wait for it: status 5 = MPLX_PLAN_INTERNAL) or placed out of probe
order (a later look-up stops at an empty slot in front of it: a duplicate again), a record compared with the wrong key, and the
hand-over into the loop.  At the default table factor (16 slots per pool state, load <= 1/16) probe paths of more than two slots
and foreign tags in them hardly occur, so the cases run at setTableFactor(1) as well: the pools are sized from the oracle's state
counts so that the table ends about a third full.  Every result word is compared with the run without helpers (whose kernel keeps
the parent's look-up) and with the CPU oracle, bit for bit.

The setter's clamp is checked without a device."""
import gc

import pytest

from mpl_ros_amd import _capi, mapgen
from oracle import orc
from tests import util
from tests.test_cached_units import SETS, _word, bmap, check_against_oracle
from tests.test_cached_units import cpu_run as jrk_cpu_run
from tests.test_helper_touch import CAP_ONE, CAP_SIX, KW, cpu_run, flood_queries, tmap

ONE_NODES, SIX_NODES, JRK_NODES = 1 << 18, 1 << 20, 1 << 15  # node pools = table slots at factor 1 (powers of two)


def test_table_factor_clamp():
    """0, negative and too large values are clamped to [1, 64] (a negative MPLX_TABLE_FACTOR, taken as unsigned, used to send the
    table's size computation round its loop for ever)"""
    lib = _capi.load()
    assert [lib.mplx_table_factor_clamp(n) for n in (0, -1, -(1 << 31), 65, (1 << 31) - 1)] == [1, 1, 1, 64, 64]
    assert [lib.mplx_table_factor_clamp(n) for n in (1, 2, 16, 64)] == [1, 2, 16, 64]


def planner(cap, n_slots, nodes, factor):
    grid, origin, res = tmap()
    gc.collect()
    mu, pl = util.make_gpu(grid, origin, res, mapgen.control_lattice(1.0, 1, True), n_slots=n_slots, max_nodes=nodes, max_edges=16 * nodes, max_log=8 * nodes, max_expand=cap, **KW)
    if factor:
        pl.setTableFactor(factor)
    return mu, pl


def run(pl, queries, control=orc.ACC):
    R = pl.planBatch([util.gpu_wp(s, control=control) for s, g in queries], [util.gpu_wp(g, control=control) for s, g in queries])
    assert pl.helperStats()["helpers_gave_up"] == 0
    assert all(r.status != 5 for r in R)  # MPLX_PLAN_INTERNAL
    return tuple(_word(pl, i, r) for i, r in enumerate(R)), sum(pl.queryCycles(i)["cache_hits"] for i in range(len(queries)))


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [1, 0], ids=["factor1", "default_factor"])
def test_one_flooding_query(factor):
    cpu = cpu_run(CAP_ONE, 0, 1)
    # (from the oracle: capped, and 87 669 states in 2^18 slots -- a table a third full at factor 1)
    assert cpu[0]["status"] == 3 and cpu[0]["n_nodes"] == 87669 and 0.3 < cpu[0]["n_nodes"] / ONE_NODES < 0.4
    queries = flood_queries()[0:1]
    mu, pl = planner(CAP_ONE, 1, ONE_NODES, factor)
    pl.setHelpers(0, -1)
    off, hits_off = run(pl, queries)
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC>" and hits_off == 0
    pl.setHelpers(4, -1)
    on, hits = run(pl, queries)
    print(f"one query, factor {factor or 16}: {on[0][1]} expansions, {on[0][3]} states, cache hits {hits}, kernel {pl.lastKernelMs():.1f} ms")
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>" and hits > 0
    assert on == off
    check_against_oracle(on, cpu)
    del mu, pl


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [1, 0], ids=["factor1", "default_factor"])
def test_six_queries_on_two_slots(factor):
    """finished and concurrent queries leave foreign tags in each other's probe paths; the pool's chunks are recycled, the table's
    entries stay"""
    cpu = cpu_run(CAP_SIX, 0, 6)
    total = sum(cpu[i]["n_nodes"] for i in range(6))
    assert all(cpu[i]["status"] == 3 for i in range(6)) and 0.3 < total / SIX_NODES < 0.5  # (every state of the six keeps its entry: 424 332)
    queries = flood_queries()
    mu, pl = planner(CAP_SIX, 2, SIX_NODES, factor)
    pl.setHelpers(0, -1)
    off, _ = run(pl, queries)
    check_against_oracle(off, cpu)
    pl.setHelpers(4, -1)
    pl.setPoolRecycling(True)
    for rep in range(2):
        on, hits = run(pl, queries)
        print(f"six queries, factor {factor or 16}, recycled, run {rep}: cache hits {hits}, kernel {pl.lastKernelMs():.1f} ms")
        assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>" and hits > 0
        assert on == off
    del mu, pl


@pytest.mark.gpu
def test_jerk_lattice_of_27_inputs_factor1():
    """the other build with units of 32 lanes, <32,16,JRK,help> (a hot line of 60 bytes: nine key integers; it keeps the unpeeled look-up,
    whose probe loop shares its source with the flagship's), on a table half full"""
    cpu = jrk_cpu_run("jrk")
    # (from the oracle: the query reaches its goal -- the trajectory is compared too -- with 16 170 states: one chunk of 2^15, half full)
    assert cpu[0]["status"] == 0 and 0.4 < cpu[0]["n_nodes"] / JRK_NODES < 0.6
    grid, origin, res = bmap()
    qf, control, kw = SETS["jrk"]
    queries = qf()
    gc.collect()
    mu, pl = util.make_gpu(grid, origin, res, mapgen.control_lattice(1.0, 1, True), n_slots=1, max_nodes=JRK_NODES, max_edges=8 * JRK_NODES, max_log=4 * JRK_NODES, **kw)
    pl.setTableFactor(1)
    pl.setHelpers(0, -1)
    off, _ = run(pl, queries, control)
    pl.setHelpers(4, -1)
    on, hits = run(pl, queries, control)
    print(f"jerk query, factor 1: {on[0][1]} expansions, {on[0][3]} states, cache hits {hits}, kernel {pl.lastKernelMs():.1f} ms")
    assert pl.kernelName() == "astar_spec_kernel<32,16,JRK,help>" and hits > 0
    assert on == off
    check_against_oracle(on, cpu)
    del mu, pl
