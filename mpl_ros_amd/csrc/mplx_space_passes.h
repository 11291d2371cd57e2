// mplx_space_passes.h -- (internal) the dimension-independent passes of a state-space export from the device pools, shared by
// mplx_poly_space.hip (2-D moving-obstacle A*) and mplx_poly3_space.hip (3-D): any search that runs on the pools, chunk tables and
// edge records of mplx_kernels.h (commit_parallel, publish_chunk_tables) can be exported through them.  What differs between the
// planners is the state row; the kernels are templates over a ROW policy
//   struct ROW { static constexpr int W;  // doubles per exported state
//                static __device__ void decode(const double *st, int nk, double *o); };  // pool state (nk doubles, then t) -> row
// Everything has internal linkage: each including unit gets its own instances and its device code depends on nothing else.
//
// The search launch has completed before anything here runs, and the kernels run on the context's stream: plain loads and stores,
// no cross-workgroup protocol, nothing of DESIGN 3.9.
//   pass 1  space_nodes_kernel<ROW> : one lane per node id -> states[n][ROW::W], g, h, flag byte, length of the predecessor list
//           space_scan_kernel       : exclusive scan of the per-tile sums of those lengths (one workgroup), total
//   pass 2  space_edges_kernel      : one lane per node walks its list again and writes (child, parent, action) at its offset, reversed
//                                     (the device list is newest first, the reference's pred vectors grow by push_back)
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_device.h"
#include "mplx_space_common.h"

namespace {

struct SpaceArgs {
  const char *node_pool, *edge_pool;
  const uint32_t *node_table, *edge_table;  // of the query
  uint32_t n_nodes, n_edges;
  uint32_t node_chunks, edge_chunks;        // pool sizes: a table entry at or above them (NIL included) names no chunk
  int32_t rb, hot, nk;                      // record bytes, hot-part bytes, state doubles
  double *states, *g, *h;
  uint8_t *flags;
  uint32_t *len, *tile_sum;                 // per node / per tile (after the scan: exclusive prefix)
  unsigned long long *total;
  uint32_t *err;
  int32_t *child, *parent, *action;
};

__device__ __forceinline__ const char *space_node(const SpaceArgs &A, uint32_t id) {
  return A.node_pool + (((size_t)A.node_table[id >> NODE_CH_LOG] << NODE_CH_LOG) + (id & ((1u << NODE_CH_LOG) - 1u))) * (size_t)A.rb;
}
__device__ __forceinline__ const uint32_t *space_edge(const SpaceArgs &A, uint32_t e) {
  return (const uint32_t *)(A.edge_pool + (((size_t)A.edge_table[e >> EDGE_CH_LOG] << EDGE_CH_LOG) + (e & ((1u << EDGE_CH_LOG) - 1u))) * (size_t)EDGE_BYTES);
}

template <typename ROW>
__global__ __launch_bounds__(TILE) void space_nodes_kernel(SpaceArgs A) {
  constexpr int W = ROW::W;
  __shared__ double st_out[TILE * W];  // the tile's states, written out in rows of consecutive doubles
  __shared__ uint32_t sc[TILE];
  const int tid = threadIdx.x;
  const uint32_t n_tiles = (A.n_nodes + TILE - 1) / TILE;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t id = tile * TILE + (uint32_t)tid;
    uint32_t cnt = 0;
    if (id < A.n_nodes) {
      if (A.node_table[id >> NODE_CH_LOG] >= A.node_chunks) {
        atomicOr(A.err, ERR_TABLE);
        for (int d = 0; d < W; d++) st_out[tid * W + d] = 0.0;
      } else {
        const char *r = space_node(A, id);
        const double *hotp = (const double *)r;
        const uint32_t *w = (const uint32_t *)(r + 16);
        const uint32_t fl = w[0];
        A.g[id] = hotp[0];
        A.h[id] = hotp[1];
        A.flags[id] = (uint8_t)(fl & (FLAG_CLOSED | FLAG_OPENED));
        ROW::decode((const double *)(r + A.hot), A.nk, st_out + tid * W);  // pos3 vel3 (acc3) t -- as mplx_ctx_ext_nodes decodes it
        // length of the predecessor list: every index below n_edges, at most n_edges steps
        for (uint32_t e = w[1]; e != NIL;) {
          if (e >= A.n_edges || cnt >= A.n_edges || A.edge_table[e >> EDGE_CH_LOG] >= A.edge_chunks) {
            atomicOr(A.err, ERR_LIST);
            break;
          }
          cnt++;
          e = space_edge(A, e)[1];
        }
        A.len[id] = cnt;
      }
    }
    uint32_t tot;
    (void)tile_excl_scan(cnt, sc, tid, tot);  // (its barriers also publish st_out)
    if (tid == 0) A.tile_sum[tile] = tot;
    const uint32_t first = tile * TILE, rows = A.n_nodes - first < (uint32_t)TILE ? A.n_nodes - first : (uint32_t)TILE;
    for (uint32_t k = tid; k < rows * (uint32_t)W; k += TILE) A.states[(size_t)first * W + k] = st_out[k];
    __syncthreads();
  }
}

// tile_sum[] -> exclusive prefix, in place; *total = sum.  One workgroup: 131072 tiles at the most (33 M states per query).
__global__ __launch_bounds__(TILE) void space_scan_kernel(SpaceArgs A) {
  __shared__ uint32_t sc[TILE];
  __shared__ unsigned long long carry;
  const int tid = threadIdx.x;
  const uint32_t n_tiles = (A.n_nodes + TILE - 1) / TILE;
  if (tid == 0) carry = 0ull;
  __syncthreads();
  for (uint32_t base = 0; base < n_tiles; base += TILE) {
    const uint32_t i = base + (uint32_t)tid;
    const uint32_t v = i < n_tiles ? A.tile_sum[i] : 0u;
    uint32_t tot;
    const uint32_t ex = tile_excl_scan(v, sc, tid, tot);
    const unsigned long long c = carry;
    if (i < n_tiles) A.tile_sum[i] = (uint32_t)(c + ex);  // (the host compares *total with n_edges before an offset is used)
    __syncthreads();
    if (tid == 0) carry = c + tot;
    __syncthreads();
  }
  if (tid == 0) *A.total = carry;
}

__global__ __launch_bounds__(TILE) void space_edges_kernel(SpaceArgs A) {
  __shared__ uint32_t sc[TILE];
  const int tid = threadIdx.x;
  const uint32_t n_tiles = (A.n_nodes + TILE - 1) / TILE;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t id = tile * TILE + (uint32_t)tid;
    const uint32_t cnt = id < A.n_nodes ? A.len[id] : 0u;
    uint32_t tot;
    const uint32_t off = A.tile_sum[tile] + tile_excl_scan(cnt, sc, tid, tot);
    if (cnt) {
      const uint32_t *w = (const uint32_t *)(space_node(A, id) + 16);
      uint32_t k = 0;
      for (uint32_t e = w[1]; e != NIL && k < cnt; k++) {
        if (e >= A.n_edges) { atomicOr(A.err, ERR_LIST); break; }
        const uint32_t *er = space_edge(A, e);  // {parent, next, action}
        const size_t at = (size_t)off + (cnt - 1u - k);
        if (at < (size_t)A.n_edges) {
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
