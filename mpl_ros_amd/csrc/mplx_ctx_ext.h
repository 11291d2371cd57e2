// mplx_ctx_ext.h -- (internal, not part of include/mplx.h) a planner context's pools and launch guard for the search kernels
// of other translation units (mplx_ctx_ext.inl, compiled into mplx_api.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mplx.h"
#include "mplx_device.h"

// starts the kernel on stream s with `grid` workgroups; false: no build for this configuration
typedef bool (*mplx_ext_launch)(void *user, int grid, hipStream_t s, const mplx::SearchParams &P);
int mplx_ctx_ext_plan(mplx_ctx *c, int n, const mplx::QueryIn *in, mplx_ext_launch launch, void *user, const char *what, mplx_result *out);
int mplx_ctx_ext_nodes(mplx_ctx *c, int q, uint64_t cap, mplx_waypoint *coords, double *g, int32_t *closed, int32_t *opened);
const char *mplx_ctx_ext_error(const mplx_ctx *c);

// Where the last batch of the context left its pools, chunk tables and per-query outcomes: what a state-space export that runs in
// another translation unit (mplx_poly3_space.hip) reads them through, as mplx_poly_space_view does for an mplx_poly handle.
struct mplx_ctx_ext_view {
  int32_t device;
  hipStream_t stream;                // the context's stream: the search launch has completed on it
  int32_t last_nq;                   // queries of the last batch (0: none, or the last launch was aborted)
  int32_t pending, pools_valid, recycled;
  int32_t pool_control;              // control kind of the pool records
  const mplx::QueryOut *last_out;    // host copy, last_nq entries
  const char *node_pool, *edge_pool;
  uint32_t node_chunks, edge_chunks;  // pool sizes in chunks
  const uint32_t *node_tables, *edge_tables;  // device: nq x MAX_NODE_CH / nq x MAX_EDGE_CH
  uint64_t plan_epoch;               // plan launches of the context so far
  mplx::GuardBlock *guard;           // the context's host-coherent launch-guard block (a kernel of another unit that runs between the
  double deadline_s;                 // context's own launches polls it) and its launch deadline (mplx_set_deadline; <= 0: none)
};
int mplx_ctx_ext_view_get(const mplx_ctx *c, mplx_ctx_ext_view *out);
