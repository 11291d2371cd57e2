"""-m gpu: units served from the look-ahead cache next to units that are not, in the builds with two units per wave.

A cached unit takes validity, the blocked flags, the heuristics and the voxel-read count from the helper's record and row; its
neighbour in the wave samples its own primitives.  The record check, the row check and the successor test of a candidate all use
one key hash, computed once per batch by the lane that checks the record and kept in LDS (mplx_spec.h, KeyHashLds::cur_hash): a hash
that is missing, stale or of the neighbouring unit refuses a good record (fewer hits, same results), polls a row until the search
ends with status 5, or misses a candidate among the successors (a different closed flag, a different plan).  The cases below put
hits and misses into the same batches (the regime is asserted from queryCycles: 0 < hits < expansions) and compare every query with
the run without helpers and with the CPU oracle on status, expansions, expansion-order hash, states, predecessor records, voxel
reads, successors, finite successors, cost and path actions.  voxel_reads is the counter a wrong hand-over reaches first: a cached
unit's count comes from the row, an uncached one's from its own sampling (node cell, samples outside the map, occupied cells).

Every shape is the 128^3 benchmark map, a 27-input lattice and a cap of at most 20 000 expansions per query."""
import functools
import gc

import numpy as np
import pytest

from mpl_ros_amd import mapgen
from oracle import orc
from tests import util
from tests.test_gpu_scale import _cpu_replay

pytestmark = pytest.mark.gpu
CAP = 20000


@functools.lru_cache(maxsize=None)
def bmap():
    grid, origin, res, _, _, _ = mapgen.benchmark_map(128)
    grid = np.ascontiguousarray(grid)
    grid.setflags(write=False)
    return grid, origin, res


@functools.lru_cache(maxsize=None)
def batch_queries():
    grid, origin, res = bmap()
    return tuple(mapgen.c4_queries(grid, origin, res, 40, rank=3, min_dist=6.0))


@functools.lru_cache(maxsize=None)
def edge_queries():
    """Two searches that run into their cap, chosen from the map alone.
    [0] starts in the cell layer x = 1 (0.15 m from the map's edge; a primitive of the lattice travels 0.5 m from rest and 2.5 m at
        v_max) and aims at a point 2 m OUTSIDE that face: the front presses against the face, the samples of most primitives fall
        outside the map (code 2, no voxel read), and so does the node-cell test's neighbourhood.
    [1] starts in a free cell whose +x neighbour is occupied and floods from there (run with eps = 0: f = g): the front runs along
        the occupied cells of every box around the start, primitives are blocked at their first samples."""
    grid, origin, res = bmap()
    n = grid.shape[0]
    mid = n // 2
    ring = sorted(((y, z) for y in range(20, n - 20) for z in range(20, n - 20)), key=lambda c: abs(c[0] - mid) + abs(c[1] - mid))
    y, z = next((y, z) for y, z in ring if grid[z, y, 1] == 0)
    s0 = (1.5 * res, (y + 0.5) * res, (z + 0.5) * res)
    g0 = (s0[0] - 2.2, s0[1], s0[2])
    occ = np.argwhere((grid[:, :, 1:] != 0) & (grid[:, :, :-1] == 0))  # (z, y, x): free cell x, occupied cell x + 1
    occ = occ[(occ[:, 2] > 30) & (occ[:, 2] < 60) & (np.abs(occ[:, 0] - mid) < 30) & (np.abs(occ[:, 1] - mid) < 30)]
    z, y, x = (int(v) for v in occ[0])
    s1 = ((x + 0.5) * res, (y + 0.5) * res, (z + 0.5) * res)
    g1 = next(((xx + 0.5) * res, s1[1], s1[2]) for xx in range(x + 50, n - 2) if grid[z, y, xx] == 0)
    return ((s0, g0), (s1, g1))


def _word(pl, i, r):
    return (r.status, r.n_expanded, r.expand_hash, r.n_nodes, r.n_edges, r.voxel_reads, r.n_succ, r.n_succ_finite, r.cost,
            tuple(pl.getTraj(i).actions.tolist()) if r.status == 0 else None)


# query set -> (queries, control, planner settings); the longest query of the batch (2950 expansions on the oracle) also runs alone
KW = dict(v_max=2.0, a_max=1.0, tol_pos=0.5)
SETS = {
    "one": (lambda: batch_queries()[36:37], orc.ACC, dict(KW, max_expand=CAP)),
    "batch": (batch_queries, orc.ACC, dict(KW, max_expand=CAP)),
    "edge": (lambda: edge_queries()[0:1], orc.ACC, dict(KW, max_expand=6000)),
    "wall": (lambda: edge_queries()[1:2], orc.ACC, dict(KW, max_expand=4000, eps=0.0)),
    "jrk": (lambda: batch_queries()[36:37], orc.JRK, dict(KW, j_max=1.0, max_expand=5000)),
}


@functools.lru_cache(maxsize=None)
def gpu_run(which, per, reserved):
    """(per-query result words, cache hits, expansions, kernel name) of one planBatch of the named query set"""
    grid, origin, res = bmap()
    qf, control, kw = SETS[which]
    queries = qf()
    nq = len(queries)
    U = mapgen.control_lattice(1.0, 1, True)
    pools = mapgen.c4_pools(False, nq, kw["max_expand"], per_q=200_000 if nq == 1 else 100_000)
    gc.collect()
    mu, pl = util.make_gpu(grid, origin, res, U, n_slots=nq, max_nodes=pools["nodes"], max_edges=pools["edges"], max_log=pools["log"], **kw)
    pl.setHelpers(per, reserved)
    R = pl.planBatch([util.gpu_wp(s, control=control) for s, g in queries], [util.gpu_wp(g, control=control) for s, g in queries])
    words = tuple(_word(pl, i, r) for i, r in enumerate(R))
    st = pl.helperStats()
    assert st["helpers_gave_up"] == 0
    hits = sum(pl.queryCycles(i)["cache_hits"] for i in range(nq))
    n_exp = sum(r.n_expanded for r in R)
    name = pl.kernelName()
    print(f"{which} helpers ({per}, {reserved}): {nq} queries, {n_exp} expansions, cache hits {hits}, kernel {name} {pl.lastKernelMs():.1f} ms")
    del mu, pl, R
    gc.collect()
    return words, hits, n_exp, name


@functools.lru_cache(maxsize=None)
def cpu_run(which):
    grid, origin, res = bmap()
    qf, control, kw = SETS[which]
    queries = list(qf())
    return _cpu_replay(grid, origin, res, control, mapgen.control_lattice(1.0, 1, True), kw, queries, list(range(len(queries))))


def check_against_oracle(words, cpu):
    for i, (st, ne, hh, nn, ned, reads, nsucc, nfin, cost, acts) in enumerate(words):
        c = cpu[i]
        assert (st, ne, hh, nn, ned, reads, nsucc, nfin) == (c["status"], c["n_expanded"], c["hash"], c["n_nodes"], c["n_edges"], c["reads"], c["n_succ"], c["n_fin"]), i
        if st == 0:
            assert cost == c["cost"] and acts == tuple(np.asarray(c["actions"]).tolist()), i


@pytest.mark.parametrize("which,per,reserved", [("one", 4, -1), ("batch", 2, 64)], ids=["one_query_four_helpers", "batch40_reserved"])
def test_mixed_batches_acc(which, per, reserved):
    """hits and misses in the same batches and waves: the helped run equals the run without helpers and the oracle"""
    on, hits, n_exp, name = gpu_run(which, per, reserved)
    off, hits_off, _, _ = gpu_run(which, 0, -1)
    assert name == "astar_spec_kernel<32,16,ACC,help>"
    assert hits_off == 0
    assert 0 < hits < n_exp  # the regime: cached and uncached units share batches
    assert on == off
    check_against_oracle(on, cpu_run(which))


@pytest.mark.parametrize("which", ["edge", "wall"])
def test_node_cell_and_boundary_paths(which):
    """a front pressed against the map's edge (samples outside the map: no voxel read) and a front along occupied cells, four
    helpers each: voxel_reads against the oracle's first, then everything else"""
    grid, origin, res = bmap()
    (s0, g0), (s1, g1) = edge_queries()
    assert s0[0] < 0.5 and g0[0] < -1.0 and grid[int(s1[2] / res), int(s1[1] / res), int(s1[0] / res) + 1] != 0  # the two situations, from the map alone
    on, hits, n_exp, name = gpu_run(which, 4, -1)
    off, _, _, _ = gpu_run(which, 0, -1)
    assert name == "astar_spec_kernel<32,16,ACC,help>"
    assert 0 < hits < n_exp
    cpu = cpu_run(which)
    assert cpu[0]["status"] == 3 and on[0][5] == cpu[0]["reads"]  # (capped; a cached unit takes voxel_reads from the row)
    assert on == off
    check_against_oracle(on, cpu)


def test_jerk_lattice_of_27_inputs():
    """the other build with two units per wave: <32,16,JRK,help>"""
    on, hits, n_exp, name = gpu_run("jrk", 4, -1)
    off, _, _, _ = gpu_run("jrk", 0, -1)
    assert name == "astar_spec_kernel<32,16,JRK,help>"
    assert 0 < hits < n_exp
    assert on == off
    check_against_oracle(on, cpu_run("jrk"))


def test_batch_without_helpers():
    """astar_spec_kernel<32,16,ACC>: the same source without the look-ahead cache (the hash is computed where it is used there)"""
    off, hits, _, name = gpu_run("batch", 0, -1)
    assert name == "astar_spec_kernel<32,16,ACC>" and hits == 0
    check_against_oracle(off, cpu_run("batch"))
