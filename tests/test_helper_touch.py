"""-m gpu: the helpers' record touch (mplx_spec.h MPLX_X_HELP_TOUCH) changes no result.

A helper of the 32-lane builds loads the home slot of every successor it finds in the served query's part of the state table and,
where the slot names a state of that query, one word of the state's record -- translated through the leader's chunk table in memory,
which the leader now keeps current while it searches.  Slot, chunk entry and record word may all be stale; they only form an address.
What could go wrong is therefore an address outside the pool (a fault), a helper that falls behind (fewer hits, same results) or a
chunk-table store that lands where it does not belong (another query's results change).  The cases run the 27-input ACC lattice on
util.small_map(112) -- the cube maps of tests/util.py were tried in steps of 16 cells: the state space of the 96^3 map is exhausted at
51 066 states, below the 65 536 the first case needs -- with helpers forced on, and compare every result word with the run without
helpers and with the CPU oracle, bit for bit.

  1. one search that creates more than 2 * 2^15 states (picked from the oracle's count): its chunk table grows twice while helpers
     serve it, and the touch counter must show that the path ran;
  2. six searches on two slots with pool recycling on, after a batch that left its chunk tables behind: chunks change hands while
     helpers translate through entries of finished queries.
The same batches on a library built with -DMPLX_X_HELP_TOUCH=0 are not run here (the harness of tests/test_cached_units.py loads no
variants): that comparison is the digests of tools/ab.py, recorded in profiles/helper_touch_speed.txt."""
import functools
import gc

import numpy as np
import pytest

from mpl_ros_amd import mapgen
from oracle import orc
from tests import util
from tests.test_cached_units import _word, check_against_oracle
from tests.test_gpu_scale import _cpu_replay

pytestmark = pytest.mark.gpu
N = 112
KW = dict(v_max=2.0, a_max=1.0, tol_pos=0.5)
CAP_ONE, CAP_SIX = 60000, 40000


@functools.lru_cache(maxsize=None)
def tmap():
    grid, origin, res = util.small_map(N)
    grid = np.ascontiguousarray(grid)
    grid.setflags(write=False)
    return grid, origin, res


@functools.lru_cache(maxsize=None)
def flood_queries():
    """Searches that cannot reach their goal -- a point 2 m outside the face x = 0 -- and flood the map until the cap: starts on
    free cells, [0] the one nearest the centre, the others spread along the diagonal."""
    grid, origin, res = tmap()
    free = np.argwhere(grid == 0)
    out = []
    for c in (N // 2, N // 4, 3 * N // 4, N // 3, 2 * N // 3, N // 2 + 9):
        z, y, x = (int(v) for v in free[np.argmin(np.abs(free - c).sum(axis=1))])
        s = ((x + 0.5) * res, (y + 0.5) * res, (z + 0.5) * res)
        out.append((s, (-2.05, s[1], s[2])))
    assert len(set(out)) == 6
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cpu_run(cap, lo, hi):
    grid, origin, res = tmap()
    queries = list(flood_queries()[lo:hi])
    return _cpu_replay(grid, origin, res, orc.ACC, mapgen.control_lattice(1.0, 1, True), dict(KW, max_expand=cap), queries, list(range(len(queries))))


def planner(cap, n_slots, nodes):
    grid, origin, res = tmap()
    gc.collect()
    return util.make_gpu(grid, origin, res, mapgen.control_lattice(1.0, 1, True), n_slots=n_slots, max_nodes=nodes, max_edges=16 * nodes, max_log=8 * nodes, max_expand=cap, **KW)


def run(pl, queries):
    R = pl.planBatch([util.gpu_wp(s) for s, g in queries], [util.gpu_wp(g) for s, g in queries])
    assert pl.helperStats()["helpers_gave_up"] == 0
    return tuple(_word(pl, i, r) for i, r in enumerate(R)), sum(pl.queryCycles(i)["cache_hits"] for i in range(len(queries)))


def test_chunk_table_grows_twice_under_the_helpers():
    cpu = cpu_run(CAP_ONE, 0, 1)
    assert cpu[0]["n_nodes"] > 2 * 32768 and cpu[0]["status"] == 3  # (the query, chosen by the oracle's state count: three chunks)
    queries = flood_queries()[0:1]
    mu, pl = planner(CAP_ONE, 1, 1 << 18)
    pl.setHelpers(0, -1)
    off, hits_off = run(pl, queries)
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC>" and hits_off == 0 and pl.helperTouches() == 0
    pl.setHelpers(4, -1)
    on, hits = run(pl, queries)
    touches = pl.helperTouches()
    print(f"one query: {on[0][1]} expansions, {on[0][3]} states, cache hits {hits}, touches {touches}, kernel {pl.lastKernelMs():.1f} ms")
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>"
    assert hits > 0 and touches > 0  # the helpers served, and the touch path ran
    assert on == off
    check_against_oracle(on, cpu)
    del mu, pl


def test_six_queries_on_two_slots_with_recycled_chunks():
    cpu = cpu_run(CAP_SIX, 0, 6)
    assert all(cpu[i]["n_nodes"] > 32768 for i in range(6))  # (every query takes more than one chunk)
    queries = flood_queries()
    mu, pl = planner(CAP_SIX, 2, 1 << 20)
    pl.setHelpers(0, -1)
    off, _ = run(pl, queries)  # (un-recycled: every query's chunk table stays behind in memory)
    check_against_oracle(off, cpu)
    pl.setHelpers(4, -1)
    pl.setPoolRecycling(True)
    for rep in range(2):
        on, hits = run(pl, queries)
        touches = pl.helperTouches()
        print(f"six queries, recycled, run {rep}: cache hits {hits}, touches {touches}, kernel {pl.lastKernelMs():.1f} ms")
        assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>"
        assert hits > 0 and touches > 0
        assert on == off
    del mu, pl
