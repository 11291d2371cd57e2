// mplx_poly3_lpa_host.h -- what the LPA* of the 3-D moving-obstacle planner (mplx_poly3_lpa.hip, a translation unit of its own) needs
// to know of an mplx_poly3 handle (mplx_poly3.hip): the device view of its committed worlds and planner set-up, its stream, the launch
// guard of its planner context.  As mplx_poly_lpa_host.h is for the 2-D planner.
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_device.h"
#include "mplx_poly3.h"

struct mplx_poly3;
struct mplx_poly3_lpa_view {
  mplx::Poly3Dev dev;       // device arrays of the committed worlds, control inputs, limits
  int32_t general;          // hyperplane equations above degree two can occur (JRK primitives / high-degree obstacle segments)
  int32_t n_worlds, device;
  hipStream_t stream;
  mplx::GuardBlock *guard;  // host-coherent launch-guard block of the handle's planner context
  double deadline_s;        // <= 0: none (mplx_poly3_set_deadline)
  uint64_t commit_epoch;    // number of mplx_poly3_commit calls so far (the worlds a kernel sees are those of the last one)
  uint64_t cfg_epoch;       // number of mplx_poly3_config calls so far
};
// MPLX_OK, or MPLX_ERR_ARG when the handle is not configured / committed (the text is in mplx_poly3_last_error)
int mplx_poly3_lpa_internal_view(mplx_poly3 *p, mplx_poly3_lpa_view *out);
