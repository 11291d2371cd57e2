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
