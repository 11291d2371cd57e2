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
  int32_t last_yaw;                  // the last plan carried yaw: a record's state is followed by the yaw, then t
  const mplx::QueryOut *last_out;    // host copy, last_nq entries
  const char *node_pool, *edge_pool;
  uint32_t node_chunks, edge_chunks;  // pool sizes in chunks
  const uint32_t *node_tables, *edge_tables;  // device: nq x MAX_NODE_CH / nq x MAX_EDGE_CH
  uint64_t plan_epoch;               // plan launches of the context so far
  mplx::GuardBlock *guard;           // the context's host-coherent launch-guard block (a kernel of another unit that runs between the
  double deadline_s;                 // context's own launches polls it) and its launch deadline (mplx_set_deadline; <= 0: none)
};
int mplx_ctx_ext_view_get(const mplx_ctx *c, mplx_ctx_ext_view *out);

// The state-space export over a list of queries of the last batch (mplx_space.hip: mplx_result_space* / mplx_cloud_result_space*).
// Its device buffers and the one cached export live in a slot of the context and are freed with it; a refused export leaves its
// text where mplx_last_error reads it (c null: where mplx_last_error(NULL) does).
struct mplx_space;
void mplx_space_free(mplx_space *s);  // (mplx_space.hip) the context's device is current
void mplx_space_invalidate(mplx_space *s);  // (mplx_space.hip) called before every search launch on the context: nothing cached is served again
mplx_space **mplx_ctx_ext_space_slot(mplx_ctx *c);
int mplx_ctx_ext_fail(mplx_ctx *c, int code, const char *msg);  // returns code
// (mplx_cloud.hip) the internal context a point-cloud planner searches on; msg -> mplx_cloud_last_error, returns code
mplx_ctx *mplx_cloud_internal_ctx(mplx_cloud *c);
int mplx_cloud_internal_fail(mplx_cloud *c, int code, const char *msg);
