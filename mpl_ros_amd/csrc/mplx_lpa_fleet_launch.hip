// mplx_lpa_fleet_launch.hip -- instantiates and launches the FLEET builds of the LPA* kernels (mplx_lpa.h): the search of N planners
// in one launch (member = blockIdx.x) and the three passes of a map edit over all of them (member = blockIdx.y).  A translation unit
// of its own, so that the single-planner kernels of mplx_lpa_launch.hip are compiled exactly as before.
#include <hip/hip_runtime.h>

#include "mplx_lpa.h"

using namespace mplx;

template <int BLOCK>
static void launch_lpa_fleet(int what, int control, hipStream_t s, const SearchParams &P, const LpaParams &A, int mode, int pass, int grid_x, int members) {
#define MPLX_LPA_FLEET_CASE(C)                                                                                                   \
  if (what == 0) hipLaunchKernelGGL((lpa_plan_kernel<BLOCK, C, true>), dim3(members), dim3(BLOCK), 0, s, P, A);                  \
  else hipLaunchKernelGGL((lpa_update_kernel<BLOCK, C, true>), dim3(grid_x, members), dim3(BLOCK), 0, s, P, A, mode, pass);
  switch (control) {
    case CTRL_VEL: MPLX_LPA_FLEET_CASE(CTRL_VEL) break;
    case CTRL_ACC: MPLX_LPA_FLEET_CASE(CTRL_ACC) break;
    case CTRL_JRK: MPLX_LPA_FLEET_CASE(CTRL_JRK) break;
    default: MPLX_LPA_FLEET_CASE(CTRL_SNP) break;
  }
#undef MPLX_LPA_FLEET_CASE
}

// what: 0 ComputeShortestPath of `members` planners, 1 map edit (mode 0 blocked / 1 cleared; pass 0..2 of lpa_update_kernel on
// grid_x workgroups per member).  A.members: one LpaMember per planner (device memory).  false: lattice too wide, or no member.
bool mplx_launch_lpa_fleet(int what, int mode, hipStream_t s, const SearchParams &P, const LpaParams &A, int pass, int grid_x, int members) {
  if (P.n_u > 128 || members < 1 || members > 65535 || grid_x < 1 || !A.members) return false;
  if (P.n_u <= 64) launch_lpa_fleet<64>(what, P.control, s, P, A, mode, pass, grid_x, members);
  else launch_lpa_fleet<128>(what, P.control, s, P, A, mode, pass, grid_x, members);
  return true;
}
