// mplx_space_common.h -- (internal) what every state-space export shares, whatever its passes: the tile, the error bits, the
// workgroup scan, the device buffer that grows on demand and the grid size.  Included by mplx_space_passes.h (one query: the 2-D and
// 3-D moving-obstacle A*, the LPA* exports) and by mplx_space_query_passes.h (a list of queries of a planner context).  No kernel
// lives here: a unit that includes this header alone gets none it does not launch.  Everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include "mplx_device.h"

namespace {

using namespace mplx;

constexpr int TILE = 256;  // nodes per workgroup pass (divides a node chunk: the records of a tile are contiguous)
static_assert(((1 << NODE_CH_LOG) % TILE) == 0, "a tile must not straddle a node chunk");
constexpr uint32_t ERR_LIST = 1u, ERR_DEGREE = 2u, ERR_TABLE = 4u;

// exclusive scan of v over the TILE lanes of the workgroup (LDS buffer sc[TILE]); total in `tot`
__device__ __forceinline__ uint32_t tile_excl_scan(uint32_t v, uint32_t *sc, int tid, uint32_t &tot) {
  sc[tid] = v;
  __syncthreads();
  for (int d = 1; d < TILE; d <<= 1) {
    const uint32_t add = tid >= d ? sc[tid - d] : 0u;
    __syncthreads();
    sc[tid] += add;
    __syncthreads();
  }
  const uint32_t incl = sc[tid];
  tot = sc[TILE - 1];
  __syncthreads();
  return incl - v;
}

template <typename T>
struct Buf {  // a device buffer that grows on demand
  T *d = nullptr;
  size_t cap = 0;
  hipError_t need(size_t n) {
    if (n <= cap) return hipSuccess;
    (void)hipFree(d);
    d = nullptr;
    cap = 0;
    hipError_t e = hipMalloc((void **)&d, sizeof(T) * n);
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() { (void)hipFree(d); d = nullptr; cap = 0; }
};

int grid_for(size_t items) { return (int)(items < 4096 ? (items ? items : 1) : 4096); }

}  // namespace
