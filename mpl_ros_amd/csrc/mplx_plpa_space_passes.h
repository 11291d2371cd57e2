// mplx_plpa_space_passes.h -- (internal) the passes of a state-space export from the pools of moving-obstacle LPA* planners
// (mplx_plpa_* / mplx_plpa3_* and their fleets), used by mplx_plpa_space.hip.  The LPA* side of mplx_space_passes.h: the same ROW
// policy (doubles per exported state, pool state -> row), the same tile and tile scan, but
//   * the pools of an LPA* handle are flat (identity chunk tables): record i lies at pool + i * bytes;
//   * every pass runs over an ARRAY of members (one descriptor per handle, separate pools) in one launch: workgroups map to
//     (member, tile) through the prefix of tile counts kept in the descriptors, the outputs are concatenated arrays with the
//     per-member offsets of the descriptors.  One handle is an array of one;
//   * a state carries rhs and the built flag, an entry carries the blocked bit.
// The search / updateNodes launch has completed before anything here runs, and the kernels run on the planner's stream: plain loads
// and stores, no cross-workgroup protocol beyond the scan of tile sums, f64 only moved.
//   nodes    plpa_space_nodes_kernel<ROW>  : one lane per state id -> row, g, rhs, h, flag byte; walks the state's predecessor list
//                                            and scatters child[entry] = id.  Every output is optional (null: not produced)
//   records  plpa_space_count_kernel       : one lane per entry, entries of a tile that pass the filter -> tile_sum
//            plpa_space_scan_kernel        : exclusive scan of tile_sum (one workgroup), total
//            plpa_space_write_kernel       : one lane per entry writes (entry, child, parent, action, blocked) at its rank: stable,
//                                            creation order kept, members one after the other
//   gather   plpa_space_gather_kernel<ROW> : one lane per listed entry -> row of the parent state, action, now-blocked bit
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_device.h"
#include "mplx_lpa.h"
#include "mplx_space_passes.h"

namespace {

constexpr uint32_t PERR_LIST = 1u, PERR_ENTRY = 2u, PERR_MEMBER = 4u;
constexpr int PLPA_WHICH_ALL = 0, PLPA_WHICH_VALID = 1, PLPA_WHICH_BLOCKED = 2;
static_assert((FLAG_CLOSED | FLAG_OPENED | FLAG_BUILT) == 7u, "the flag byte holds closed / opened / built");

struct PlpaSpaceMember {
  const char *node_pool, *edge_pool;
  uint32_t n_nodes, n_edges;
  int32_t rb, hot, nk;                    // record bytes, hot-part bytes, state doubles
  uint32_t node_tile0, edge_tile0;        // the member's first tile in the sequence of state tiles / entry tiles
  uint32_t pad;
  unsigned long long node_off, edge_off;  // the member's first row in the concatenated per-state / per-entry arrays
};

struct PlpaSpaceArgs {
  const PlpaSpaceMember *members;
  int32_t n_members;
  uint32_t node_tiles, edge_tiles;
  uint32_t *err;
  // nodes pass (null: not produced)
  double *states, *g, *rhs, *h;
  uint8_t *flags;
  int32_t *child;                         // per entry (all members, at edge_off)
  // records passes
  int32_t which;
  uint32_t *tile_sum;                     // per entry tile (after the scan: exclusive prefix)
  unsigned long long *total;
  unsigned long long *member_first;       // per member with entries: rank of its first record
  unsigned long long rec_cap;             // rows the record arrays hold
  int32_t *r_entry, *r_child, *r_parent, *r_action, *r_blocked;
};

struct PlpaGatherArgs {
  PlpaSpaceMember m;
  const uint32_t *items;                  // entry number | now-blocked << 31
  uint32_t n_items;
  uint32_t *err;
  double *rows;
  int32_t *action, *now_blocked;
};

// the member a tile belongs to: the last one whose first tile is not above it (members without tiles share their successor's)
template <bool EDGE>
__device__ __forceinline__ int plpa_member_of(const PlpaSpaceArgs &A, uint32_t tile) {
  int lo = 0, hi = A.n_members - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const uint32_t t0 = EDGE ? A.members[mid].edge_tile0 : A.members[mid].node_tile0;
    if (t0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename ROW>
__global__ __launch_bounds__(TILE) void plpa_space_nodes_kernel(PlpaSpaceArgs A) {
  constexpr int W = ROW::W;
  __shared__ double st_out[TILE * W];  // the tile's states, written out in rows of consecutive doubles
  const int tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < A.node_tiles; tile += gridDim.x) {
    const PlpaSpaceMember M = A.members[plpa_member_of<false>(A, tile)];
    const uint32_t first = (tile - M.node_tile0) * (uint32_t)TILE;
    if (tile < M.node_tile0 || first >= M.n_nodes) {  // (uniform) the descriptors do not cover this tile
      if (tid == 0) atomicOr(A.err, PERR_MEMBER);
      continue;
    }
    const uint32_t id = first + (uint32_t)tid;
    if (id < M.n_nodes) {
      const char *r = M.node_pool + (size_t)id * (size_t)M.rb;
      const double *hotp = (const double *)r;
      const uint32_t *w = (const uint32_t *)(r + 16);
      const double *st = (const double *)(r + M.hot);
      const size_t at = (size_t)M.node_off + id;
      if (A.g) A.g[at] = hotp[0];
      if (A.h) A.h[at] = hotp[1];
      if (A.rhs) A.rhs[at] = st[M.nk + 1];
      if (A.flags) A.flags[at] = (uint8_t)(w[0] & (FLAG_CLOSED | FLAG_OPENED | FLAG_BUILT));
      if (A.states) ROW::decode(st, M.nk, st_out + tid * W);
      if (A.child) {
        // the state's predecessor list: every index below n_edges, at most n_edges steps
        uint32_t cnt = 0;
        for (uint32_t e = w[1]; e != NIL;) {
          if (e >= M.n_edges || cnt >= M.n_edges) {
            atomicOr(A.err, PERR_LIST);
            break;
          }
          cnt++;
          A.child[(size_t)M.edge_off + e] = (int32_t)id;
          e = ((const uint32_t *)(M.edge_pool + (size_t)e * EDGE_BYTES))[1];
        }
      }
    }
    if (A.states) {  // (uniform)
      __syncthreads();
      const uint32_t rows = M.n_nodes - first < (uint32_t)TILE ? M.n_nodes - first : (uint32_t)TILE;
      double *out = A.states + ((size_t)M.node_off + first) * W;
      for (uint32_t k = tid; k < rows * (uint32_t)W; k += TILE) out[k] = st_out[k];
      __syncthreads();
    }
  }
}

// entry e of the member at lane `tid` of an entry tile: its record and whether the filter keeps it
__device__ __forceinline__ bool plpa_entry_keep(const PlpaSpaceMember &M, uint32_t e, int which, uint32_t &parent, uint32_t &action) {
  if (e >= M.n_edges) return false;
  const uint32_t *er = (const uint32_t *)(M.edge_pool + (size_t)e * EDGE_BYTES);  // {parent, next, action | EDGE_BLOCKED}
  parent = er[0];
  action = er[2];
  const bool blocked = (action & EDGE_BLOCKED) != 0u;
  return which == PLPA_WHICH_ALL || (which == PLPA_WHICH_BLOCKED) == blocked;
}

__global__ __launch_bounds__(TILE) void plpa_space_count_kernel(PlpaSpaceArgs A) {
  const int tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < A.edge_tiles; tile += gridDim.x) {
    const PlpaSpaceMember M = A.members[plpa_member_of<true>(A, tile)];
    uint32_t parent = 0, action = 0;
    bool keep = false;
    if (tile >= M.edge_tile0) keep = plpa_entry_keep(M, (tile - M.edge_tile0) * (uint32_t)TILE + (uint32_t)tid, A.which, parent, action);
    const int tot = __syncthreads_count(keep ? 1 : 0);
    if (tid == 0) A.tile_sum[tile] = (uint32_t)tot;
  }
}

// tile_sum[] -> exclusive prefix, in place; *total = sum.  One workgroup.
__global__ __launch_bounds__(TILE) void plpa_space_scan_kernel(PlpaSpaceArgs A) {
  __shared__ uint32_t sc[TILE];
  __shared__ unsigned long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0ull;
  __syncthreads();
  for (uint32_t base = 0; base < A.edge_tiles; base += TILE) {
    const uint32_t i = base + (uint32_t)tid;
    const uint32_t v = i < A.edge_tiles ? A.tile_sum[i] : 0u;
    uint32_t tot;
    const uint32_t ex = tile_excl_scan(v, sc, tid, tot);
    const unsigned long long c = carry;
    if (i < A.edge_tiles) A.tile_sum[i] = (uint32_t)(c + ex);  // (below 2^32: the host refuses more entries than that in one call)
    __syncthreads();
    if (tid == 0) carry = c + tot;
    __syncthreads();
  }
  if (tid == 0) *A.total = carry;
}

__global__ __launch_bounds__(TILE) void plpa_space_write_kernel(PlpaSpaceArgs A) {
  __shared__ uint32_t sc[TILE];
  const int tid = threadIdx.x;
  for (uint32_t tile = blockIdx.x; tile < A.edge_tiles; tile += gridDim.x) {
    const int mi = plpa_member_of<true>(A, tile);
    const PlpaSpaceMember M = A.members[mi];
    uint32_t parent = 0, action = 0;
    bool keep = false;
    const uint32_t e = (tile - M.edge_tile0) * (uint32_t)TILE + (uint32_t)tid;
    if (tile >= M.edge_tile0) keep = plpa_entry_keep(M, e, A.which, parent, action);
    uint32_t tot;
    const uint32_t base = A.tile_sum[tile];
    const size_t at = (size_t)base + tile_excl_scan(keep ? 1u : 0u, sc, tid, tot);
    if (tid == 0 && tile == M.edge_tile0) A.member_first[mi] = base;
    if (keep) {
      if (at < (size_t)A.rec_cap) {
        if (A.r_entry) A.r_entry[at] = (int32_t)e;
        if (A.r_child) A.r_child[at] = A.child[(size_t)M.edge_off + e];
        if (A.r_parent) A.r_parent[at] = (int32_t)parent;
        if (A.r_action) A.r_action[at] = (int32_t)(action & ~EDGE_BLOCKED);
        if (A.r_blocked) A.r_blocked[at] = (action & EDGE_BLOCKED) ? 1 : 0;
      } else {
        atomicOr(A.err, PERR_ENTRY);
      }
    }
  }
}

template <typename ROW>
__global__ __launch_bounds__(TILE) void plpa_space_gather_kernel(PlpaGatherArgs G) {
  constexpr int W = ROW::W;
  __shared__ double st_out[TILE * W];
  const int tid = threadIdx.x;
  const uint32_t n_tiles = (G.n_items + TILE - 1) / TILE;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t first = tile * (uint32_t)TILE, i = first + (uint32_t)tid;
    if (i < G.n_items) {
      const uint32_t c = G.items[i], e = c & 0x7FFFFFFFu;
      uint32_t parent = NIL, action = 0;
      if (e < G.m.n_edges) {
        const uint32_t *er = (const uint32_t *)(G.m.edge_pool + (size_t)e * EDGE_BYTES);
        parent = er[0];
        action = er[2];
      }
      if (parent < G.m.n_nodes) {
        const char *r = G.m.node_pool + (size_t)parent * (size_t)G.m.rb;
        if (G.rows) ROW::decode((const double *)(r + G.m.hot), G.m.nk, st_out + tid * W);
      } else {
        atomicOr(G.err, PERR_ENTRY);
        if (G.rows)
          for (int d = 0; d < W; d++) st_out[tid * W + d] = 0.0;
      }
      if (G.action) G.action[i] = (int32_t)(action & ~EDGE_BLOCKED);
      if (G.now_blocked) G.now_blocked[i] = (int32_t)(c >> 31);
    }
    if (G.rows) {  // (uniform)
      __syncthreads();
      const uint32_t rows = G.n_items - first < (uint32_t)TILE ? G.n_items - first : (uint32_t)TILE;
      double *out = G.rows + (size_t)first * W;
      for (uint32_t k = tid; k < rows * (uint32_t)W; k += TILE) out[k] = st_out[k];
      __syncthreads();
    }
  }
}

}  // namespace
