// mplx_cloud_prior.hip -- the point-cloud search guided by prior trajectories (P-list of mplx_cloud.h): the prior-aware
// instantiations of the cloud A* and the parity entry of its heuristic.  A translation unit of its own, so that the search
// without a prior (mplx_cloud.hip) is compiled exactly as before; the C-ABI around both is in mplx_cloud.hip.
#include <hip/hip_runtime.h>

#define MPLX_CLOUD_SEARCH_ONLY
#include "mplx_cloud.h"

using namespace mplx;

// P2 for K states (13 doubles each, masked to the control kind by the host) against one goal and one table
__global__ void cloud_heuristic_kernel(int control, HeurParams hp, double dt, CloudPriorView R, int K, const double *states, double *h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  State s;
  for (int k = 0; k < 12; k++) ((double *)&s)[k] = states[13 * (size_t)i + k];
  int32_t key[MAX_KEY];
  const int nk = state_key(control, s, key);
  h[i] = cloud_prior_heur(hp, control, s, key, nk, states[13 * (size_t)i + 12], dt, R);
}

void mplx_cloud_heuristic_launch(hipStream_t s, int control, const HeurParams &hp, double dt, const CloudPriorView &R, int K, const double *states, double *h) {
  hipLaunchKernelGGL(cloud_heuristic_kernel, dim3((K + 127) / 128), dim3(128), 0, s, control, hp, dt, R, K, states, h);
}

bool mplx_cloud_prior_launch(int grid, hipStream_t s, const SearchParams &P, const CloudDev &D, const CloudPriorDev &PR) {
  switch (P.control) {
    case CTRL_VEL: hipLaunchKernelGGL((astar_cloud_prior_kernel<256, CTRL_VEL>), dim3(grid), dim3(256), 0, s, P, D, PR); return true;
    case CTRL_ACC: hipLaunchKernelGGL((astar_cloud_prior_kernel<256, CTRL_ACC>), dim3(grid), dim3(256), 0, s, P, D, PR); return true;
    case CTRL_JRK: hipLaunchKernelGGL((astar_cloud_prior_kernel<256, CTRL_JRK>), dim3(grid), dim3(256), 0, s, P, D, PR); return true;
    case CTRL_SNP: hipLaunchKernelGGL((astar_cloud_prior_kernel<256, CTRL_SNP>), dim3(grid), dim3(256), 0, s, P, D, PR); return true;
    default: return false;
  }
}
