// mplx_poly_space.hip -- the state space of a query of the last mplx_poly_plan_batch, exported ON THE DEVICE straight from the pools
// (C-ABI mplx_poly_result_nodes / _edges / _blocked, include/mplx.h): PlannerBase::getCloseSet / getOpenSet / getValidPrimitives /
// getAllPrimitives of the batched 2-D moving-obstacle A*.  A translation unit of its own: the device code of every other unit stays
// what it is.
//
// The search launch has completed (guard_wait + stream synchronisation in mplx_poly_plan_batch) before anything here runs, and the
// kernels run on the context's stream: plain loads and stores, no cross-workgroup protocol, nothing of DESIGN 3.9.
//   pass 1  space_nodes_kernel<Row2> : one lane per node id -> states[n][9], g, h, flag byte, length of the predecessor list
//           space_scan_kernel        : exclusive scan of the per-tile sums of those lengths (one workgroup), total
//   pass 2  space_edges_kernel       : one lane per node walks its list again and writes (child, parent, action) at its offset, reversed
//   (mplx_space_passes.h: shared with the 3-D export, mplx_poly3_space.hip)
//   pass 3  poly_space_blocked_kernel<GEN> : one 64-lane workgroup per closed node re-derives env_poly_map::get_succ (D7: the batched A*
//                                     does not materialise blocked successors) -> one mask word per node, bit a = input a is blocked
// One export per (plan epoch, q) is kept on the device: _nodes, _edges and _blocked of the same query do not repeat an earlier pass, and
// only what the caller asked for crosses the bus.
#include "../../include/mplx.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "mplx_poly_space.h"
#include "mplx_space_passes.h"

using namespace mplx;

namespace {

// the exported row of a 2-D state: pos2 vel2 acc2 jrk2 t out of the pool's pos3 vel3 (acc3) t
struct Row2 {
  static constexpr int W = 9;
  static __device__ __forceinline__ void decode(const double *st, int nk, double *o) {
    o[0] = st[0]; o[1] = st[1];
    o[2] = st[3]; o[3] = st[4];
    o[4] = nk >= 9 ? st[6] : 0.0; o[5] = nk >= 9 ? st[7] : 0.0;
    o[6] = 0.0; o[7] = 0.0;
    o[8] = st[nk];
  }
};

// env_poly_map::get_succ of the closed states of query q, as poly_get_succ_kernel (mplx_poly_search.h) runs it -- the state comes from
// the pool record, the world is world_of[q], t_rel = t - W.start_t -- with one word per node as the outcome: bit a is set iff primitive a
// is valid (end point inside the bounding box, validate_primitive) and isFree(start.pos, t) or isFree(pr, t) failed.
template <bool GEN>
__global__ __launch_bounds__(64) void poly_space_blocked_kernel(PolyDev D, SpaceArgs A, const int32_t *world_of, int q, uint32_t *mask) {
  constexpr int BLOCK = 64;
  __shared__ double cs[POLY_MAX_U][2][6];
  __shared__ int32_t valid[POLY_MAX_U], hit[POLY_MAX_U];
  __shared__ int32_t start_hit, unsupported, hp_max;
  __shared__ PolyPrep prep[POLY_MAX_OBS];
  __shared__ uint32_t hit_idx[POLY_MAX_U * POLY_MAX_OBS], uns_idx[POLY_MAX_U * POLY_MAX_OBS];
  const int tid = threadIdx.x;
  const PolyWorld W = D.worlds[world_of[q]];
  for (uint32_t id = blockIdx.x; id < A.n_nodes; id += gridDim.x) {
    if (!(A.flags[id] & FLAG_CLOSED)) {  // (uniform) not expanded: the search never asked get_succ of it
      if (tid == 0) mask[id] = 0u;
      continue;
    }
    const double *st = (const double *)(space_node(A, id) + A.hot);
    const double T = D.dt, t_rel = st[A.nk] - W.start_t;
    if (tid == 0) { start_hit = 0; unsupported = 0; }
    if (tid < D.n_u) {
      const double pos[2] = {st[0], st[1]}, vel[2] = {st[3], st[4]}, acc[2] = {A.nk >= 9 ? st[6] : 0.0, A.nk >= 9 ? st[7] : 0.0}, u[2] = {D.U[2 * tid], D.U[2 * tid + 1]};
      double c[2][6];
      poly_prim_build(D.control, pos, vel, u, c, acc);
      for (int i = 0; i < 2; i++)
        for (int j = 0; j < 6; j++) cs[tid][i][j] = c[i][j];
      const double ex = pp_p_auto(c[0], T), ey = pp_p_auto(c[1], T);
      valid[tid] = (poly_inside(W.bbox, 4, ex, ey) && poly_validate(D.control, c, T, D.v_max, D.a_max, D.j_max)) ? 1 : 0;
      hit[tid] = 0;
    }
    __syncthreads();
    poly_collide_all<BLOCK, PolyNoHook, GEN>(D, W, cs, valid, D.n_u, T, t_rel, prep, hit_idx, uns_idx, &hp_max, hit, &unsupported, &start_hit, tid, 0, PolyNoHook());
    const bool b = tid < D.n_u && valid[tid] && (start_hit || hit[tid]);
    const unsigned long long m = __ballot(b);  // (one wave: POLY_MAX_U = 32 inputs, bit 31 included)
    if (tid == 0) {
      mask[id] = (uint32_t)m;
      if (unsupported) atomicOr(A.err, ERR_DEGREE);
    }
    __syncthreads();
  }
}

}  // namespace

struct mplx_poly_space {
  // what the buffers hold: query q of plan launch `epoch`, passes done so far
  uint64_t epoch = 0;
  int32_t q = -1;
  bool have_nodes = false, have_edges = false, have_blocked = false;
  uint64_t n_blocked = 0;
  std::vector<uint32_t> masks;  // host copy of the blocked masks (4 bytes per state)
  Buf<double> states, g, h;
  Buf<uint8_t> flags;
  Buf<uint32_t> len, tile_sum, mask;
  Buf<int32_t> child, parent, action;
  Buf<unsigned long long> total;  // [0] scan total, [1] (low word) error bits
  // (measurement) kernel time of the last nodes + scan / edges / blocked pass that ran
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float ms[3] = {0, 0, 0};
};
void mplx_poly_space_free(mplx_poly_space *s) {
  if (!s) return;
  s->states.release(); s->g.release(); s->h.release(); s->flags.release(); s->len.release(); s->tile_sum.release(); s->mask.release();
  s->child.release(); s->parent.release(); s->action.release(); s->total.release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
}

namespace {

#define SCHK(p, call)                                                                  \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess) {                                                           \
      char b__[384];                                                                   \
      snprintf(b__, sizeof(b__), "%s failed: %s", #call, hipGetErrorString(e__));      \
      return mplx_poly_space_internal_fail((p), MPLX_ERR_HIP, b__);                    \
    }                                                                                  \
  } while (0)

int sfail(mplx_poly *p, int code, const char *msg) { return mplx_poly_space_internal_fail(p, code, msg); }

// Checks common to the three getters.  *n_nodes = 0: nothing to serve (MPLX_OK).
int space_open(mplx_poly *p, int32_t q, mplx_poly_space_view &V, const QueryOut *&o) {
  if (!p) return MPLX_ERR_ARG;
  if (int r = mplx_poly_space_internal_view(p, &V)) return r;
  if (V.pending) return sfail(p, MPLX_ERR_ARG, "a submitted batch is still outstanding on this context (mplx_plan_batch_wait first)");
  if (q < 0 || q >= V.last_nq) return sfail(p, MPLX_ERR_ARG, "no such query in the last mplx_poly_plan_batch");
  o = &V.last_out[q];
  if (o->n_nodes == 0) return MPLX_OK;  // an occupied start, a start at the goal: no state was created
  if (!V.pools_valid || V.recycled) return sfail(p, MPLX_ERR_ARG, "the pools of the last batch were released: its state spaces are gone");
  if (o->status == MPLX_PLAN_POOL_FULL || o->status == MPLX_PLAN_INTERNAL) {
    char b[256];
    snprintf(b, sizeof(b), "query %d ended with status %d (%s): its last records may be half built, the state space is not served", q, o->status,
             o->status == MPLX_PLAN_POOL_FULL ? "MPLX_PLAN_POOL_FULL" : "MPLX_PLAN_INTERNAL");
    return sfail(p, MPLX_ERR_ARG, b);
  }
  if (o->status != MPLX_PLAN_OK && o->status != MPLX_PLAN_NO_PATH && o->status != MPLX_PLAN_MAX_EXPAND && o->status != MPLX_PLAN_TRAJ_TOO_LONG)
    return sfail(p, MPLX_ERR_ARG, "the query did not leave a consistent state space");
  if (o->n_nodes > ((unsigned long long)MAX_NODE_CH << NODE_CH_LOG) || o->n_edges > ((unsigned long long)MAX_EDGE_CH << EDGE_CH_LOG))
    return sfail(p, MPLX_ERR_ARG, "inconsistent state-space counts");
  SCHK(p, hipSetDevice(V.device));
  return MPLX_OK;
}

SpaceArgs space_args(const mplx_poly_space_view &V, const mplx_poly_space &S, int32_t q, const QueryOut &o) {
  SpaceArgs A{};
  A.node_pool = V.node_pool; A.edge_pool = V.edge_pool;
  A.node_table = V.node_tables + (size_t)q * MAX_NODE_CH;
  A.edge_table = V.edge_tables + (size_t)q * MAX_EDGE_CH;
  A.n_nodes = (uint32_t)o.n_nodes; A.n_edges = (uint32_t)o.n_edges;
  A.node_chunks = V.node_chunks; A.edge_chunks = V.edge_chunks;
  A.rb = rec_bytes(V.pool_control); A.hot = rec_hot_bytes(V.pool_control); A.nk = state_len(V.pool_control);
  A.states = S.states.d; A.g = S.g.d; A.h = S.h.d; A.flags = S.flags.d; A.len = S.len.d; A.tile_sum = S.tile_sum.d;
  A.total = S.total.d; A.err = (uint32_t *)(S.total.d + 1);
  A.child = S.child.d; A.parent = S.parent.d; A.action = S.action.d;
  return A;
}

int space_err(mplx_poly *p, mplx_poly_space &S, uint32_t err) {
  S.q = -1;  // nothing of this export is kept
  if (err & ERR_TABLE) return sfail(p, MPLX_ERR_ARG, "inconsistent chunk table");
  if (err & ERR_DEGREE) return sfail(p, MPLX_ERR_ARG, "internal: a hyperplane equation of degree > 2 was met by the quadratic-only kernel");
  return sfail(p, MPLX_ERR_ARG, "corrupt predecessor list");
}

// pass 1 (once per (plan epoch, q)): states, g, h, flags, list lengths, their scan
int space_nodes(mplx_poly *p, const mplx_poly_space_view &V, int32_t q, const QueryOut &o, mplx_poly_space *&S) {
  if (!*V.space) *V.space = new mplx_poly_space();
  S = *V.space;
  if (S->q == q && S->epoch == V.plan_epoch && S->have_nodes) return MPLX_OK;
  S->q = -1;
  S->have_nodes = S->have_edges = S->have_blocked = false;
  const size_t n = (size_t)o.n_nodes, n_tiles = (n + TILE - 1) / TILE;
  SCHK(p, S->states.need(n * 9)); SCHK(p, S->g.need(n)); SCHK(p, S->h.need(n)); SCHK(p, S->flags.need(n)); SCHK(p, S->len.need(n));
  SCHK(p, S->tile_sum.need(n_tiles)); SCHK(p, S->total.need(2));
  const SpaceArgs A = space_args(V, *S, q, o);
  if (!S->ev0) { SCHK(p, hipEventCreate(&S->ev0)); SCHK(p, hipEventCreate(&S->ev1)); }
  SCHK(p, hipMemsetAsync(S->total.d, 0, 2 * sizeof(unsigned long long), V.stream));
  SCHK(p, hipEventRecord(S->ev0, V.stream));
  hipLaunchKernelGGL(space_nodes_kernel<Row2>, dim3(grid_for(n_tiles)), dim3(TILE), 0, V.stream, A);
  hipLaunchKernelGGL(space_scan_kernel, dim3(1), dim3(TILE), 0, V.stream, A);
  SCHK(p, hipGetLastError());
  SCHK(p, hipEventRecord(S->ev1, V.stream));
  unsigned long long back[2] = {0, 0};
  SCHK(p, hipMemcpyAsync(back, S->total.d, sizeof(back), hipMemcpyDeviceToHost, V.stream));
  SCHK(p, hipStreamSynchronize(V.stream));
  SCHK(p, hipEventElapsedTime(&S->ms[0], S->ev0, S->ev1));
  if ((uint32_t)back[1]) return space_err(p, *S, (uint32_t)back[1]);
  if (back[0] != o.n_edges) {
    char b[256];
    snprintf(b, sizeof(b), "corrupt predecessor list: the lists of query %d hold %llu records, the search counted %llu", q, back[0], (unsigned long long)o.n_edges);
    return sfail(p, MPLX_ERR_ARG, b);
  }
  S->q = q;
  S->epoch = V.plan_epoch;
  S->have_nodes = true;
  return MPLX_OK;
}

}  // namespace

extern "C" int mplx_poly_result_nodes(mplx_poly *p, int32_t q, uint64_t cap, double *states, double *g, double *h, int32_t *closed, int32_t *opened) {
  mplx_poly_space_view V;
  const QueryOut *o = nullptr;
  if (int r = space_open(p, q, V, o)) return r;
  const size_t n = (size_t)o->n_nodes;
  if (n == 0) return MPLX_OK;
  if ((uint64_t)n > cap) {
    char b[256];
    snprintf(b, sizeof(b), "state-space dump: query %d created %zu states, the caller's arrays hold %llu", q, n, (unsigned long long)cap);
    return sfail(p, MPLX_ERR_CAPACITY, b);
  }
  mplx_poly_space *S = nullptr;
  if (int r = space_nodes(p, V, q, *o, S)) return r;
  std::vector<uint8_t> fl;
  if (states) SCHK(p, hipMemcpyAsync(states, S->states.d, sizeof(double) * 9 * n, hipMemcpyDeviceToHost, V.stream));
  if (g) SCHK(p, hipMemcpyAsync(g, S->g.d, sizeof(double) * n, hipMemcpyDeviceToHost, V.stream));
  if (h) SCHK(p, hipMemcpyAsync(h, S->h.d, sizeof(double) * n, hipMemcpyDeviceToHost, V.stream));
  if (closed || opened) {
    fl.resize(n);
    SCHK(p, hipMemcpyAsync(fl.data(), S->flags.d, n, hipMemcpyDeviceToHost, V.stream));
  }
  SCHK(p, hipStreamSynchronize(V.stream));
  if (closed)
    for (size_t i = 0; i < n; i++) closed[i] = (fl[i] & FLAG_CLOSED) ? 1 : 0;
  if (opened)
    for (size_t i = 0; i < n; i++) opened[i] = (fl[i] & FLAG_OPENED) ? 1 : 0;
  return MPLX_OK;
}

extern "C" int mplx_poly_result_edges(mplx_poly *p, int32_t q, uint64_t cap, int32_t *child, int32_t *parent, int32_t *action, uint64_t *n_out) {
  if (n_out) *n_out = 0;
  mplx_poly_space_view V;
  const QueryOut *o = nullptr;
  if (int r = space_open(p, q, V, o)) return r;
  if (o->n_nodes == 0) return MPLX_OK;
  mplx_poly_space *S = nullptr;
  if (int r = space_nodes(p, V, q, *o, S)) return r;  // (the scan total has been checked against n_edges)
  const size_t ne = (size_t)o->n_edges;
  if (n_out) *n_out = ne;
  const size_t cnt = cap < (uint64_t)ne ? (size_t)cap : ne;
  if (cnt == 0 || (!child && !parent && !action)) return MPLX_OK;
  if (!S->have_edges) {
    SCHK(p, S->child.need(ne)); SCHK(p, S->parent.need(ne)); SCHK(p, S->action.need(ne));
    const SpaceArgs A = space_args(V, *S, q, *o);
    SCHK(p, hipEventRecord(S->ev0, V.stream));
    hipLaunchKernelGGL(space_edges_kernel, dim3(grid_for(((size_t)o->n_nodes + TILE - 1) / TILE)), dim3(TILE), 0, V.stream, A);
    SCHK(p, hipGetLastError());
    SCHK(p, hipEventRecord(S->ev1, V.stream));
    unsigned long long back[2] = {0, 0};
    SCHK(p, hipMemcpyAsync(back, S->total.d, sizeof(back), hipMemcpyDeviceToHost, V.stream));
    SCHK(p, hipStreamSynchronize(V.stream));
    SCHK(p, hipEventElapsedTime(&S->ms[1], S->ev0, S->ev1));
    if ((uint32_t)back[1]) return space_err(p, *S, (uint32_t)back[1]);
    S->have_edges = true;
  }
  if (child) SCHK(p, hipMemcpyAsync(child, S->child.d, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, V.stream));
  if (parent) SCHK(p, hipMemcpyAsync(parent, S->parent.d, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, V.stream));
  if (action) SCHK(p, hipMemcpyAsync(action, S->action.d, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, V.stream));
  SCHK(p, hipStreamSynchronize(V.stream));
  return MPLX_OK;
}

extern "C" int mplx_poly_result_blocked(mplx_poly *p, int32_t q, uint64_t cap, int32_t *parent, int32_t *action, uint64_t *n_out) {
  if (n_out) *n_out = 0;
  mplx_poly_space_view V;
  const QueryOut *o = nullptr;
  if (int r = space_open(p, q, V, o)) return r;
  if (o->n_nodes == 0) return MPLX_OK;
  // get_succ is a pure function of state, lattice, limits and world: re-derived only against what the plan ran with
  if (V.cfg_epoch != V.plan_cfg_epoch)
    return sfail(p, MPLX_ERR_ARG, "the planner was re-configured since the plan (mplx_poly_config): its blocked primitives cannot be re-derived");
  if (V.commit_epoch != V.plan_commit_epoch)
    return sfail(p, MPLX_ERR_ARG, "the worlds were committed again since the plan (mplx_poly_commit): its blocked primitives cannot be re-derived (they would be computed against the new worlds)");
  mplx_poly_space *S = nullptr;
  if (int r = space_nodes(p, V, q, *o, S)) return r;
  const size_t n = (size_t)o->n_nodes;
  if (!S->have_blocked) {
    SCHK(p, S->mask.need(n));
    const SpaceArgs A = space_args(V, *S, q, *o);
    SCHK(p, hipEventRecord(S->ev0, V.stream));
    if (V.general)
      hipLaunchKernelGGL((poly_space_blocked_kernel<true>), dim3(grid_for(n)), dim3(64), 0, V.stream, V.dev, A, V.world_of, (int)q, S->mask.d);
    else
      hipLaunchKernelGGL((poly_space_blocked_kernel<false>), dim3(grid_for(n)), dim3(64), 0, V.stream, V.dev, A, V.world_of, (int)q, S->mask.d);
    SCHK(p, hipGetLastError());
    SCHK(p, hipEventRecord(S->ev1, V.stream));
    unsigned long long back[2] = {0, 0};
    S->masks.resize(n);
    SCHK(p, hipMemcpyAsync(S->masks.data(), S->mask.d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, V.stream));
    SCHK(p, hipMemcpyAsync(back, S->total.d, sizeof(back), hipMemcpyDeviceToHost, V.stream));
    SCHK(p, hipStreamSynchronize(V.stream));
    SCHK(p, hipEventElapsedTime(&S->ms[2], S->ev0, S->ev1));
    if ((uint32_t)back[1]) return space_err(p, *S, (uint32_t)back[1]);
    uint64_t nb = 0;
    for (size_t i = 0; i < n; i++) nb += (uint64_t)__builtin_popcount(S->masks[i]);
    S->n_blocked = nb;
    S->have_blocked = true;
  }
  if (n_out) *n_out = S->n_blocked;
  if (cap == 0 || (!parent && !action)) return MPLX_OK;
  uint64_t w = 0;
  for (size_t i = 0; i < n && w < cap; i++)
    for (uint32_t m = S->masks[i]; m && w < cap; m &= m - 1u) {  // parents in id order, actions ascending
      if (parent) parent[w] = (int32_t)i;
      if (action) action[w] = __builtin_ctz(m);
      w++;
    }
  return MPLX_OK;
}

// (measurement) kernel time of the last first pass (nodes + scan), edges pass and blocked pass that ran on the handle
extern "C" int mplx_poly_result_space_ms(mplx_poly *p, float ms[3]) {
  mplx_poly_space_view V;
  if (!p || !ms || mplx_poly_space_internal_view(p, &V) != MPLX_OK) return MPLX_ERR_ARG;
  for (int k = 0; k < 3; k++) ms[k] = *V.space ? (*V.space)->ms[k] : 0.0f;
  return MPLX_OK;
}
