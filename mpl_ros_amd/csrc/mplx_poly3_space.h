// mplx_poly3_space.h -- (internal, not part of include/mplx.h) what the state-space export of the 3-D moving-obstacle A*
// (mplx_poly3_space.hip, a translation unit of its own) needs to know of an mplx_poly3 handle (mplx_poly3.hip): the device view of the
// worlds and the planner set-up of the last plan, the context whose pools hold the last batch (mplx_ctx_ext_view), the world every
// query of that batch planned in, and the epochs that tell whether a re-derivation of get_succ would still run against the planned world.
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_ctx_ext.h"
#include "mplx_poly3.h"

struct mplx_poly3;
struct mplx_poly3_space;  // scratch buffers and the one cached export; owned by the handle, freed in mplx_poly3_destroy
struct mplx_poly3_space_view {
  mplx::Poly3Dev dev;                // device arrays of the worlds as committed last, control inputs, limits
  int32_t general;                   // the GEN choice of the last plan's search launch (poly3_general at that time)
  const mplx_ctx *ctx;               // pools, chunk tables and outcomes of the last batch
  const int32_t *plan_world_of;      // host: world of each query of the last plan (mplx_poly3_get_succ_batch re-uses the device copy)
  int32_t plan_n;                    // its length
  uint64_t commit_epoch, plan_commit_epoch;  // mplx_poly3_commit calls so far / at the last plan
  uint64_t cfg_epoch, plan_cfg_epoch;        // mplx_poly3_config calls so far / at the last plan
  mplx_poly3_space **space;          // the handle's slot for the export state
};
int mplx_poly3_space_internal_view(mplx_poly3 *p, mplx_poly3_space_view *out);
int mplx_poly3_space_internal_fail(mplx_poly3 *p, int code, const char *msg);  // leaves msg in mplx_poly3_last_error, returns code
void mplx_poly3_space_free(mplx_poly3_space *s);  // (mplx_poly3_space.hip) the handle's device is current
