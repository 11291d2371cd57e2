// mplx_poly_space.h -- (internal, not part of include/mplx.h) what the state-space export of the batched moving-obstacle A*
// (mplx_poly_space.hip, a translation unit of its own) needs to know of an mplx_poly handle (mplx_poly.inl): where the last batch's
// pools, chunk tables and per-query outcomes lie, the device view of the worlds, and the epochs that tell whether a re-derivation of
// get_succ would still run against the planned world.
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_device.h"

struct mplx_poly;
struct mplx_poly_space;  // scratch buffers and the one cached export; owned by the handle, freed in mplx_poly_destroy
struct mplx_poly_space_view {
  mplx::PolyDev dev;                 // device arrays of the worlds as committed last, control inputs, limits
  int32_t general;                   // hyperplane equations above degree two can occur (as mplx_launch_poly_get_succ's `general`)
  int32_t device;
  hipStream_t stream;                // the context's stream: the search launch has completed on it
  int32_t last_nq;                   // queries of the last batch (0: none, or the last launch was aborted)
  int32_t pending, pools_valid, recycled;
  int32_t pool_control;              // control kind of the pool records
  const mplx::QueryOut *last_out;    // host copy, last_nq entries
  const char *node_pool, *edge_pool;
  uint32_t node_chunks, edge_chunks;  // pool sizes in chunks
  const uint32_t *node_tables, *edge_tables;  // device: nq x MAX_NODE_CH / nq x MAX_EDGE_CH
  const int32_t *world_of;           // device: world of each query of the last batch
  uint64_t plan_epoch;               // plan launches of the handle so far
  uint64_t commit_epoch, plan_commit_epoch;  // mplx_poly_commit calls so far / at the last plan
  uint64_t cfg_epoch, plan_cfg_epoch;        // mplx_poly_config calls so far / at the last plan
  mplx_poly_space **space;           // the handle's slot for the export state
};
int mplx_poly_space_internal_view(mplx_poly *p, mplx_poly_space_view *out);
int mplx_poly_space_internal_fail(mplx_poly *p, int code, const char *msg);  // leaves msg in mplx_poly_last_error, returns code
void mplx_poly_space_free(mplx_poly_space *s);  // (mplx_poly_space.hip) the handle's device is current
