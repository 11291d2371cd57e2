"""-m gpu: the row of a look-ahead hit kept whole from its request to its uses (mplx_spec.h MPLX_X_ROW_TRAVEL) changes no result.

A unit of 32 lanes that takes a look-ahead hit asks for the helper's row in 2a and now keeps the row's last word -- voxel-read count |
check word -- a whole 64-bit value until it is used: behind the unit scans (S.u_reads), in the row check and in its poll loop.  The
wait for the row thereby moves from the request to the first use, behind the expansion.

What can go wrong there: a voxel-read count taken from the wrong half of the word or from a word that was never loaded (voxel_reads
differs from the oracle's -- it is the one counter whose value travels through the changed code), and a row check that compares
against a stale word (status 5 = MPLX_PLAN_INTERNAL after its polls run out, or a heuristic of another state: another expansion
order).  Every case runs with helpers and without; every result word of the two runs must be equal and equal to the CPU oracle's,
bit for bit, and the helped run must have taken look-ahead hits, so that the path is the one under test.  Nothing here delays a
helper's stores: a late row is not provoked."""
import gc

import pytest

from mpl_ros_amd import mapgen
from oracle import orc
from tests import util
from tests.test_cached_units import SETS, _word, bmap, check_against_oracle
from tests.test_cached_units import cpu_run as jrk_cpu_run
from tests.test_helper_touch import CAP_ONE, CAP_SIX, KW, cpu_run, flood_queries, tmap

pytestmark = pytest.mark.gpu
READS = 5  # position of voxel_reads in a result word (tests/test_cached_units.py _word)


def planner(cap, n_slots, nodes):
    grid, origin, res = tmap()
    gc.collect()
    return util.make_gpu(grid, origin, res, mapgen.control_lattice(1.0, 1, True), n_slots=n_slots, max_nodes=nodes, max_edges=16 * nodes, max_log=8 * nodes, max_expand=cap, **KW)


def run(pl, queries, control=orc.ACC):
    R = pl.planBatch([util.gpu_wp(s, control=control) for s, g in queries], [util.gpu_wp(g, control=control) for s, g in queries])
    assert pl.helperStats()["helpers_gave_up"] == 0
    assert all(r.status != 5 for r in R)  # MPLX_PLAN_INTERNAL
    return tuple(_word(pl, i, r) for i, r in enumerate(R)), sum(pl.queryCycles(i)["cache_hits"] for i in range(len(queries)))


def same_words(on, off, cpu):
    assert [w[READS] for w in on] == [cpu[i]["reads"] for i in range(len(on))]  # (voxel_reads first: the counter this change takes from the row at another moment)
    assert on == off
    check_against_oracle(on, cpu)


def test_one_flooding_query():
    cpu = cpu_run(CAP_ONE, 0, 1)
    assert cpu[0]["status"] == 3 and cpu[0]["n_expanded"] == CAP_ONE  # (from the oracle: the query floods the map until its cap)
    queries = flood_queries()[0:1]
    mu, pl = planner(CAP_ONE, 1, 1 << 18)
    pl.setHelpers(0, -1)
    off, hits_off = run(pl, queries)
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC>" and hits_off == 0
    pl.setHelpers(4, -1)
    on, hits = run(pl, queries)
    print(f"one query: {on[0][1]} expansions, {on[0][3]} states, voxel reads {on[0][READS]}, cache hits {hits}, kernel {pl.lastKernelMs():.1f} ms")
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>" and hits > 0
    same_words(on, off, cpu)
    del mu, pl


def test_six_queries_on_two_slots_recycled():
    """a leader that takes one query after another while helpers of the previous one detach, on recycled chunks: rows of finished
    queries stay in the look-ahead cache next to the running ones"""
    cpu = cpu_run(CAP_SIX, 0, 6)
    assert all(cpu[i]["status"] == 3 for i in range(6))
    queries = flood_queries()
    mu, pl = planner(CAP_SIX, 2, 1 << 20)
    pl.setHelpers(0, -1)
    off, hits_off = run(pl, queries)
    assert pl.kernelName() == "astar_spec_kernel<32,16,ACC>" and hits_off == 0
    pl.setHelpers(4, -1)
    pl.setPoolRecycling(True)
    for rep in range(2):
        on, hits = run(pl, queries)
        print(f"six queries, recycled, run {rep}: voxel reads {[w[READS] for w in on]}, cache hits {hits}, kernel {pl.lastKernelMs():.1f} ms")
        assert pl.kernelName() == "astar_spec_kernel<32,16,ACC,help>" and hits > 0
        same_words(on, off, cpu)
    del mu, pl


def test_jerk_lattice_of_27_inputs():
    """the other build with units of 32 lanes, <32,16,JRK,help>: the same row request and row check, nine key integers"""
    cpu = jrk_cpu_run("jrk")
    assert cpu[0]["status"] == 0  # (from the oracle: the query reaches its goal -- the trajectory is compared too)
    grid, origin, res = bmap()
    qf, control, kw = SETS["jrk"]
    queries = qf()
    pools = mapgen.c4_pools(False, 1, kw["max_expand"], per_q=200_000)
    gc.collect()
    mu, pl = util.make_gpu(grid, origin, res, mapgen.control_lattice(1.0, 1, True), n_slots=1, max_nodes=pools["nodes"], max_edges=pools["edges"], max_log=pools["log"], **kw)
    pl.setHelpers(0, -1)
    off, hits_off = run(pl, queries, control)
    assert hits_off == 0
    pl.setHelpers(4, -1)
    on, hits = run(pl, queries, control)
    print(f"jerk query: {on[0][1]} expansions, {on[0][3]} states, voxel reads {on[0][READS]}, cache hits {hits}, kernel {pl.lastKernelMs():.1f} ms")
    assert pl.kernelName() == "astar_spec_kernel<32,16,JRK,help>" and hits > 0
    same_words(on, off, cpu)
    del mu, pl
