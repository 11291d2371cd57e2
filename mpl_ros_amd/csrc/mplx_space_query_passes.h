// mplx_space_query_passes.h -- (internal) the passes of a state-space export from the pools of a planner context, over a LIST OF QUERIES
// of its last batch in one launch per pass; used by mplx_space.hip (mplx_result_space* / mplx_cloud_result_space*).  What
// mplx_space_passes.h does for one query, arranged as mplx_plpa_space_passes.h arranges the members of a fleet:
//   * one descriptor per listed query: its rows of the chunk tables (publish_chunk_tables), n_nodes, n_edges, its first tile, its
//     first row in the concatenated per-state and per-record outputs;
//   * a workgroup maps to (query, tile) through the prefix of tile counts kept in the descriptors; a query without states has no tile.
//     One query is a list of one;
//   * the tile sums and their scan are 64-bit: the offsets count the records of the whole list.
// The ROW policy gains the yaw flag of the search: struct ROW { static constexpr int W;
//                                                              static __device__ void decode(const double *st, int nk, int yaw, double *o); };
// The search launch has completed before anything here runs, and the kernels run on the context's stream: plain loads and stores, no
// cross-workgroup protocol beyond the scan of tile sums, f64 only moved, every loop bounded by a count.
//   pass 1  spaceq_nodes_kernel<ROW> : one lane per node id -> row (through LDS), g, h, flag byte, length of the predecessor list
//           spaceq_scan_kernel       : exclusive scan of the tile sums (one workgroup), total, and for every query with tiles the offset
//                                      of its first tile: the host compares it with the query's first record row before pass 2 runs
//   pass 2  spaceq_edges_kernel      : one lane per node walks its list again and writes (child, parent, action) at its offset, reversed
//                                      (the device list is newest first, the reference's pred vectors grow by push_back); nothing is
//                                      written outside the query's own segment
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_device.h"
#include "mplx_space_common.h"

namespace {

constexpr uint32_t ERR_QUERY = 8u;  // (with ERR_LIST / ERR_DEGREE / ERR_TABLE of mplx_space_common.h) the descriptors do not cover a tile

struct SpaceQuery {
  const uint32_t *node_table, *edge_table;  // the query's rows of the context's chunk tables
  uint32_t n_nodes, n_edges;
  uint32_t tile0;                           // the query's first tile in the sequence of all tiles
  int32_t q;                                // its index in the batch
  unsigned long long node_off, edge_off;    // its first row in the concatenated per-state / per-record arrays
};

struct SpaceQArgs {
  const SpaceQuery *qs;
  int32_t n_q;
  uint32_t n_tiles;
  const char *node_pool, *edge_pool;
  uint32_t node_chunks, edge_chunks;        // pool sizes: a table entry at or above them (NIL included) names no chunk
  int32_t rb, hot, nk, yaw;                 // record bytes, hot-part bytes, state doubles, 1: a yaw follows the state
  double *states, *g, *h;
  uint8_t *flags;
  uint32_t *len;                            // per state: length of its predecessor list
  unsigned long long *tile_sum;             // per tile (after the scan: exclusive prefix = record row of the tile's first entry)
  unsigned long long *total;
  unsigned long long *q_first;              // per query with tiles: the scanned offset of its first tile
  uint32_t *err;
  int32_t *child, *parent, *action;
};

// the query a tile belongs to: the last one whose first tile is not above it (queries without tiles share their successor's)
__device__ __forceinline__ int spaceq_query_of(const SpaceQArgs &A, uint32_t tile) {
  int lo = 0, hi = A.n_q - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (A.qs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ const char *spaceq_node(const SpaceQArgs &A, const SpaceQuery &Q, uint32_t id) {
  return A.node_pool + (((size_t)Q.node_table[id >> NODE_CH_LOG] << NODE_CH_LOG) + (id & ((1u << NODE_CH_LOG) - 1u))) * (size_t)A.rb;
}
__device__ __forceinline__ const uint32_t *spaceq_edge(const SpaceQArgs &A, const SpaceQuery &Q, uint32_t e) {
  return (const uint32_t *)(A.edge_pool + (((size_t)Q.edge_table[e >> EDGE_CH_LOG] << EDGE_CH_LOG) + (e & ((1u << EDGE_CH_LOG) - 1u))) * (size_t)EDGE_BYTES);
}

// exclusive scan of v over the TILE lanes of the workgroup (LDS buffer sc[TILE]); total in `tot`
__device__ __forceinline__ unsigned long long tile_excl_scan64(unsigned long long v, unsigned long long *sc, int tid, unsigned long long &tot) {
  sc[tid] = v;
  __syncthreads();
  for (int d = 1; d < TILE; d <<= 1) {
    const unsigned long long add = tid >= d ? sc[tid - d] : 0ull;
    __syncthreads();
    sc[tid] += add;
    __syncthreads();
  }
  const unsigned long long incl = sc[tid];
  tot = sc[TILE - 1];
  __syncthreads();
  return incl - v;
}

template <typename ROW>
__global__ __launch_bounds__(TILE) void spaceq_nodes_kernel(SpaceQArgs A) {
  constexpr int W = ROW::W;
  __shared__ double st_out[TILE * W];  // the tile's states, written out in rows of consecutive doubles
  __shared__ unsigned long long sc[TILE];
  const int tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const SpaceQuery Q = A.qs[spaceq_query_of(A, tile)];
    const uint32_t first = (tile - Q.tile0) * (uint32_t)TILE;
    if (tile < Q.tile0 || first >= Q.n_nodes) {  // (uniform) the descriptors do not cover this tile
      if (tid == 0) {
        atomicOr(A.err, ERR_QUERY);
        A.tile_sum[tile] = 0ull;
      }
      continue;
    }
    const uint32_t id = first + (uint32_t)tid;
    uint32_t cnt = 0;
    if (id < Q.n_nodes) {
      const size_t at = (size_t)Q.node_off + id;
      if (Q.node_table[id >> NODE_CH_LOG] >= A.node_chunks) {
        atomicOr(A.err, ERR_TABLE);
        for (int d = 0; d < W; d++) st_out[tid * W + d] = 0.0;
      } else {
        const char *r = spaceq_node(A, Q, id);
        const double *hotp = (const double *)r;
        const uint32_t *w = (const uint32_t *)(r + 16);
        A.g[at] = hotp[0];
        A.h[at] = hotp[1];
        A.flags[at] = (uint8_t)(w[0] & (FLAG_CLOSED | FLAG_OPENED));
        ROW::decode((const double *)(r + A.hot), A.nk, A.yaw, st_out + tid * W);
        // length of the predecessor list: every index below n_edges, at most n_edges steps
        for (uint32_t e = w[1]; e != NIL;) {
          if (e >= Q.n_edges || cnt >= Q.n_edges || Q.edge_table[e >> EDGE_CH_LOG] >= A.edge_chunks) {
            atomicOr(A.err, ERR_LIST);
            break;
          }
          cnt++;
          e = spaceq_edge(A, Q, e)[1];
        }
      }
      A.len[at] = cnt;
    }
    unsigned long long tot;
    (void)tile_excl_scan64(cnt, sc, tid, tot);  // (its barriers also publish st_out)
    if (tid == 0) A.tile_sum[tile] = tot;
    const uint32_t rows = Q.n_nodes - first < (uint32_t)TILE ? Q.n_nodes - first : (uint32_t)TILE;
    double *out = A.states + ((size_t)Q.node_off + first) * W;
    for (uint32_t k = tid; k < rows * (uint32_t)W; k += TILE) out[k] = st_out[k];
    __syncthreads();
  }
}

// tile_sum[] -> exclusive prefix, in place; *total = sum; q_first[i] = prefix at the first tile of query i.  One workgroup.
__global__ __launch_bounds__(TILE) void spaceq_scan_kernel(SpaceQArgs A) {
  __shared__ unsigned long long sc[TILE];
  __shared__ unsigned long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0ull;
  __syncthreads();
  for (uint32_t base = 0; base < A.n_tiles; base += TILE) {
    const uint32_t i = base + (uint32_t)tid;
    const unsigned long long v = i < A.n_tiles ? A.tile_sum[i] : 0ull;
    unsigned long long tot;
    const unsigned long long ex = tile_excl_scan64(v, sc, tid, tot);
    const unsigned long long c = carry;
    if (i < A.n_tiles) {
      A.tile_sum[i] = c + ex;
      const int qi = spaceq_query_of(A, i);
      if (A.qs[qi].tile0 == i) A.q_first[qi] = c + ex;
    }
    __syncthreads();
    if (tid == 0) carry = c + tot;
    __syncthreads();
  }
  if (tid == 0) *A.total = carry;
}

__global__ __launch_bounds__(TILE) void spaceq_edges_kernel(SpaceQArgs A) {
  __shared__ unsigned long long sc[TILE];
  const int tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const SpaceQuery Q = A.qs[spaceq_query_of(A, tile)];
    const uint32_t first = (tile - Q.tile0) * (uint32_t)TILE;
    if (tile < Q.tile0 || first >= Q.n_nodes) {  // (uniform)
      if (tid == 0) atomicOr(A.err, ERR_QUERY);
      continue;
    }
    const uint32_t id = first + (uint32_t)tid;
    const uint32_t cnt = id < Q.n_nodes ? A.len[(size_t)Q.node_off + id] : 0u;
    unsigned long long tot;
    const unsigned long long off = A.tile_sum[tile] + tile_excl_scan64(cnt, sc, tid, tot);
    if (cnt) {
      const uint32_t *w = (const uint32_t *)(spaceq_node(A, Q, id) + 16);  // (a state with a list passed the table check of pass 1)
      uint32_t k = 0;
      for (uint32_t e = w[1]; e != NIL && k < cnt; k++) {
        if (e >= Q.n_edges || Q.edge_table[e >> EDGE_CH_LOG] >= A.edge_chunks) { atomicOr(A.err, ERR_LIST); break; }
        const uint32_t *er = spaceq_edge(A, Q, e);  // {parent, next, action}
        const unsigned long long at = off + (cnt - 1u - k);
        if (at >= Q.edge_off && at - Q.edge_off < (unsigned long long)Q.n_edges) {  // inside the query's own segment
          A.child[at] = (int32_t)id;
          A.parent[at] = (int32_t)er[0];
          A.action[at] = (int32_t)(er[2] & EDGE_ACTION_MASK);
        } else {
          atomicOr(A.err, ERR_LIST);
        }
        e = er[1];
      }
    }
  }
}

}  // namespace
