// mplx_space.hip -- the state spaces of a list of queries of a planner context's last batch, exported ON THE DEVICE straight from the
// pools (C-ABI mplx_result_space* and mplx_cloud_result_space*, include/mplx_space.h): PlannerBase::getCloseSet / getOpenSet /
// getValidPrimitives / getAllPrimitives of the voxel-map A* and of the point-cloud planner, for one query or many.  A translation unit
// of its own: the device code of every other unit stays what it is.  The passes are those of mplx_space_query_passes.h, in two row
// widths: 14 columns for the voxel context (pos3 vel3 acc3 jrk3 yaw t), 13 for the cloud (pos3 vel3 acc3 jrk3 t).
//
// The search launch has completed (guard_wait + stream synchronisation in plan_batch_finish / mplx_ctx_ext_plan) before anything here
// runs, and the kernels run on the context's stream.  Every query of a batch took its pool chunks fresh (no recycling: refused
// otherwise) and its chunk tables were published per query, so the records of all of them are still in place.
// One export per (plan epoch, query list) is kept on the device, in a slot of the context: _space and _edges of the same list do not
// repeat an earlier pass, a states-only caller never runs the edges pass, and only what the caller asked for crosses the bus.
#include "../../include/mplx.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "mplx_ctx_ext.h"
#include "mplx_space_query_passes.h"

using namespace mplx;

namespace {

// the exported row of a voxel-map state: pos3 vel3 acc3 jrk3 yaw t out of the pool's state_len(control) doubles, then the yaw of a
// yaw-carrying search only, then t -- as mplx_result_nodes decodes it
struct Row14 {
  static constexpr int W = 14;
  static __device__ __forceinline__ void decode(const double *st, int nk, int yaw, double *o) {
    for (int k = 0; k < 12; k++) o[k] = k < nk ? st[k] : 0.0;
    o[12] = yaw ? st[nk] : 0.0;
    o[13] = st[nk + (yaw ? 1 : 0)];
  }
};
// the exported row of a point-cloud state: pos3 vel3 acc3 jrk3 t -- as mplx_ctx_ext_nodes decodes it
struct Row13 {
  static constexpr int W = 13;
  static __device__ __forceinline__ void decode(const double *st, int nk, int, double *o) {
    for (int k = 0; k < 12; k++) o[k] = k < nk ? st[k] : 0.0;
    o[12] = st[nk];
  }
};

}  // namespace

struct mplx_space {
  // what the buffers hold: the queries `qs` of plan launch `epoch` in rows of `width` doubles, passes done so far
  uint64_t epoch = 0;
  int width = 0;
  std::vector<int32_t> qs;
  bool have_nodes = false, have_edges = false;
  std::vector<SpaceQuery> desc_host;  // (source of the asynchronous upload)
  std::vector<unsigned long long> back;  // [0] scan total, [1] (low word) error bits, [2 + i] offset of the first tile of query i
  Buf<SpaceQuery> desc;
  Buf<double> states, g, h;
  Buf<uint8_t> flags;
  Buf<uint32_t> len;
  Buf<unsigned long long> tile_sum, ctl;
  Buf<int32_t> child, parent, action;
  // (measurement) kernel time of the last nodes + scan / edges pass that ran
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float ms[2] = {0, 0};
};
void mplx_space_free(mplx_space *s) {
  if (!s) return;
  s->desc.release(); s->states.release(); s->g.release(); s->h.release(); s->flags.release(); s->len.release(); s->tile_sum.release();
  s->ctl.release(); s->child.release(); s->parent.release(); s->action.release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
}

void mplx_space_invalidate(mplx_space *s) {
  if (s) s->have_nodes = s->have_edges = false;
}

namespace {

// whose export this is: a voxel context, or the internal context of a point-cloud planner (the refusal's text goes to its owner)
struct Target {
  mplx_ctx *ctx;
  mplx_cloud *cloud;
  bool is_cloud;
};
int sfail(const Target &T, int code, const char *msg) {
  return T.is_cloud ? mplx_cloud_internal_fail(T.cloud, code, msg) : mplx_ctx_ext_fail(T.ctx, code, msg);
}

#define SCHK(T, call)                                                                  \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess) {                                                           \
      char b__[384];                                                                   \
      snprintf(b__, sizeof(b__), "%s failed: %s", #call, hipGetErrorString(e__));      \
      return sfail((T), MPLX_ERR_HIP, b__);                                            \
    }                                                                                  \
  } while (0)

struct Open {  // a checked query list
  mplx_ctx_ext_view C;
  std::vector<int32_t> qs;
  std::vector<uint64_t> node_off, edge_off;  // n_q + 1
};

// Checks common to all entry points; launches nothing, writes nothing.
int space_open(const Target &T, int32_t n_q, const int32_t *qs, Open &O) {
  if (T.is_cloud ? !T.cloud : !T.ctx) return sfail(T, MPLX_ERR_ARG, "null handle");
  if (!T.ctx || mplx_ctx_ext_view_get(T.ctx, &O.C) != MPLX_OK) return sfail(T, MPLX_ERR_ARG, "the handle has no planner context");
  if (O.C.pending) return sfail(T, MPLX_ERR_ARG, "a submitted batch is still outstanding on this context (mplx_plan_batch_wait first)");
  if (O.C.last_nq <= 0) return sfail(T, MPLX_ERR_ARG, "state-space export: no batch has been planned on this context, or its last launch was aborted");
  if (!O.C.pools_valid) return sfail(T, MPLX_ERR_ARG, "the pools of the last batch were released (mplx_release_pools): its state spaces are gone");
  if (O.C.recycled)
    return sfail(T, MPLX_ERR_ARG, "the last batch ran with pool recycling (mplx_set_pool_recycling): the state spaces of its queries were handed back to the pools");
  if (n_q <= 0) return sfail(T, MPLX_ERR_ARG, "state-space export: the query list is empty (n_q <= 0)");
  char b[256];
  std::vector<char> seen((size_t)O.C.last_nq, 0);
  O.qs.clear();
  O.node_off.assign(1, 0);
  O.edge_off.assign(1, 0);
  for (int32_t i = 0; i < n_q; i++) {  // (a list longer than the batch ends at its first duplicate or out-of-range entry)
    const int32_t q = qs ? qs[i] : i;
    if (q < 0 || q >= O.C.last_nq) {
      snprintf(b, sizeof(b), "state-space export: no query %d in the last batch of %d", q, O.C.last_nq);
      return sfail(T, MPLX_ERR_ARG, b);
    }
    if (seen[(size_t)q]) {
      snprintf(b, sizeof(b), "state-space export: query %d is listed twice", q);
      return sfail(T, MPLX_ERR_ARG, b);
    }
    seen[(size_t)q] = 1;
    O.qs.push_back(q);
    const QueryOut &o = O.C.last_out[q];
    if (o.n_nodes) {  // (an occupied start, a start inside the goal tolerance: no state was created, whatever the status)
      if (o.status == MPLX_PLAN_POOL_FULL || o.status == MPLX_PLAN_INTERNAL) {
        snprintf(b, sizeof(b), "query %d ended with status %d (%s): its last records may be half built, the state space is not served", q, o.status,
                 o.status == MPLX_PLAN_POOL_FULL ? "MPLX_PLAN_POOL_FULL" : "MPLX_PLAN_INTERNAL");
        return sfail(T, MPLX_ERR_ARG, b);
      }
      if (o.status != MPLX_PLAN_OK && o.status != MPLX_PLAN_NO_PATH && o.status != MPLX_PLAN_MAX_EXPAND && o.status != MPLX_PLAN_TRAJ_TOO_LONG) {
        snprintf(b, sizeof(b), "query %d (status %d) did not leave a consistent state space", q, o.status);
        return sfail(T, MPLX_ERR_ARG, b);
      }
      if (o.n_nodes > ((unsigned long long)MAX_NODE_CH << NODE_CH_LOG) || o.n_edges > ((unsigned long long)MAX_EDGE_CH << EDGE_CH_LOG)) {
        snprintf(b, sizeof(b), "query %d: inconsistent state-space counts", q);
        return sfail(T, MPLX_ERR_ARG, b);
      }
    }
    O.node_off.push_back(O.node_off.back() + (o.n_nodes ? o.n_nodes : 0ull));
    O.edge_off.push_back(O.edge_off.back() + (o.n_nodes ? o.n_edges : 0ull));
  }
  if ((O.node_off[(size_t)n_q] + TILE - 1) / TILE + (uint64_t)n_q > 0x7FFFFFFFull) return sfail(T, MPLX_ERR_ARG, "state-space export: too many states for one call");
  return MPLX_OK;
}

SpaceQArgs space_args(const Open &O, const mplx_space &S, int width, uint32_t n_tiles) {
  SpaceQArgs A{};
  A.qs = S.desc.d; A.n_q = (int32_t)O.qs.size(); A.n_tiles = n_tiles;
  A.node_pool = O.C.node_pool; A.edge_pool = O.C.edge_pool;
  A.node_chunks = O.C.node_chunks; A.edge_chunks = O.C.edge_chunks;
  A.rb = rec_bytes(O.C.pool_control); A.hot = rec_hot_bytes(O.C.pool_control); A.nk = state_len(O.C.pool_control);
  A.yaw = (width == Row14::W && O.C.last_yaw) ? 1 : 0;
  A.states = S.states.d; A.g = S.g.d; A.h = S.h.d; A.flags = S.flags.d; A.len = S.len.d; A.tile_sum = S.tile_sum.d;
  A.total = S.ctl.d; A.err = (uint32_t *)(S.ctl.d + 1); A.q_first = S.ctl.d + 2;
  A.child = S.child.d; A.parent = S.parent.d; A.action = S.action.d;
  return A;
}

int space_err(const Target &T, mplx_space &S, uint32_t err) {
  S.have_nodes = S.have_edges = false;  // nothing of this export is kept
  if (err & ERR_TABLE) return sfail(T, MPLX_ERR_ARG, "inconsistent chunk table");
  if (err & ERR_QUERY) return sfail(T, MPLX_ERR_ARG, "internal: the query descriptors of the state-space export do not cover its tiles");
  return sfail(T, MPLX_ERR_ARG, "corrupt predecessor list");
}

uint32_t tiles_of(const Open &O) {
  uint64_t t = 0;
  for (size_t i = 0; i < O.qs.size(); i++) t += (O.node_off[i + 1] - O.node_off[i] + TILE - 1) / TILE;
  return (uint32_t)t;
}

// pass 1 (once per (plan epoch, query list)): states, g, h, flags, list lengths, their scan; the lists of every query hold exactly
// the records the search counted, or the export is refused.  The list creates at least one state.
int space_nodes(const Target &T, const Open &O, int width, mplx_space *&S) {
  mplx_space **slot = mplx_ctx_ext_space_slot(T.ctx);
  if (!*slot) *slot = new mplx_space();
  S = *slot;
  if (S->have_nodes && S->epoch == O.C.plan_epoch && S->width == width && S->qs == O.qs) return MPLX_OK;
  S->have_nodes = S->have_edges = false;
  const size_t n_q = O.qs.size(), n = (size_t)O.node_off[n_q];
  const uint32_t n_tiles = tiles_of(O);
  SCHK(T, hipSetDevice(O.C.device));
  SCHK(T, S->desc.need(n_q)); SCHK(T, S->states.need(n * (size_t)width)); SCHK(T, S->g.need(n)); SCHK(T, S->h.need(n)); SCHK(T, S->flags.need(n));
  SCHK(T, S->len.need(n)); SCHK(T, S->tile_sum.need(n_tiles)); SCHK(T, S->ctl.need(2 + n_q));
  if (!S->ev0) { SCHK(T, hipEventCreate(&S->ev0)); SCHK(T, hipEventCreate(&S->ev1)); }
  S->desc_host.resize(n_q);
  uint32_t tile0 = 0;
  for (size_t i = 0; i < n_q; i++) {
    const int32_t q = O.qs[i];
    SpaceQuery &D = S->desc_host[i];
    D.node_table = O.C.node_tables + (size_t)q * MAX_NODE_CH;
    D.edge_table = O.C.edge_tables + (size_t)q * MAX_EDGE_CH;
    D.n_nodes = (uint32_t)(O.node_off[i + 1] - O.node_off[i]);
    D.n_edges = (uint32_t)(O.edge_off[i + 1] - O.edge_off[i]);
    D.tile0 = tile0;
    D.q = q;
    D.node_off = O.node_off[i];
    D.edge_off = O.edge_off[i];
    tile0 += (D.n_nodes + TILE - 1) / TILE;
  }
  hipStream_t st = O.C.stream;
  const SpaceQArgs A = space_args(O, *S, width, n_tiles);
  SCHK(T, hipMemcpyAsync(S->desc.d, S->desc_host.data(), sizeof(SpaceQuery) * n_q, hipMemcpyHostToDevice, st));
  SCHK(T, hipMemsetAsync(S->ctl.d, 0, sizeof(unsigned long long) * (2 + n_q), st));
  SCHK(T, hipEventRecord(S->ev0, st));
  if (width == Row14::W)
    hipLaunchKernelGGL(spaceq_nodes_kernel<Row14>, dim3(grid_for(n_tiles)), dim3(TILE), 0, st, A);
  else
    hipLaunchKernelGGL(spaceq_nodes_kernel<Row13>, dim3(grid_for(n_tiles)), dim3(TILE), 0, st, A);
  hipLaunchKernelGGL(spaceq_scan_kernel, dim3(1), dim3(TILE), 0, st, A);
  SCHK(T, hipGetLastError());
  SCHK(T, hipEventRecord(S->ev1, st));
  S->back.assign(2 + n_q, 0ull);
  SCHK(T, hipMemcpyAsync(S->back.data(), S->ctl.d, sizeof(unsigned long long) * (2 + n_q), hipMemcpyDeviceToHost, st));
  SCHK(T, hipStreamSynchronize(st));
  SCHK(T, hipEventElapsedTime(&S->ms[0], S->ev0, S->ev1));
  if ((uint32_t)S->back[1]) return space_err(T, *S, (uint32_t)S->back[1]);
  // the records of query i start where the host put them, those of all end where the host's total does: every query's lists hold
  // exactly its n_edges records
  unsigned long long end = S->back[0];
  for (size_t i = n_q; i-- > 0;) {
    if (O.node_off[i + 1] == O.node_off[i]) continue;
    const unsigned long long first = S->back[2 + i];
    if (first != O.edge_off[i] || end != O.edge_off[i + 1]) {
      char b[256];
      snprintf(b, sizeof(b), "corrupt predecessor list: the lists of query %d hold %llu records, the search counted %llu", O.qs[i], end - first,
               (unsigned long long)(O.edge_off[i + 1] - O.edge_off[i]));
      return sfail(T, MPLX_ERR_ARG, b);
    }
    end = first;
  }
  S->qs = O.qs;
  S->epoch = O.C.plan_epoch;
  S->width = width;
  S->have_nodes = true;
  return MPLX_OK;
}

int space_counts(const Target &T, int32_t n_q, const int32_t *qs, uint64_t *node_off, uint64_t *edge_off) {
  Open O;
  if (int r = space_open(T, n_q, qs, O)) return r;
  for (int32_t i = 0; i <= n_q; i++) {
    if (node_off) node_off[i] = O.node_off[(size_t)i];
    if (edge_off) edge_off[i] = O.edge_off[(size_t)i];
  }
  return MPLX_OK;
}

int space_states(const Target &T, int width, int32_t n_q, const int32_t *qs, uint64_t cap, double *states, double *g, double *h, int32_t *closed,
                 int32_t *opened) {
  Open O;
  if (int r = space_open(T, n_q, qs, O)) return r;
  const size_t n = (size_t)O.node_off[(size_t)n_q];
  if ((uint64_t)n > cap) {
    char b[256];
    snprintf(b, sizeof(b), "state-space export: the listed queries created %zu states, the caller's arrays hold %llu", n, (unsigned long long)cap);
    return sfail(T, MPLX_ERR_CAPACITY, b);
  }
  if (n == 0) return MPLX_OK;
  mplx_space *S = nullptr;
  if (int r = space_nodes(T, O, width, S)) return r;
  hipStream_t st = O.C.stream;
  std::vector<uint8_t> fl;
  if (states) SCHK(T, hipMemcpyAsync(states, S->states.d, sizeof(double) * (size_t)width * n, hipMemcpyDeviceToHost, st));
  if (g) SCHK(T, hipMemcpyAsync(g, S->g.d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  if (h) SCHK(T, hipMemcpyAsync(h, S->h.d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  if (closed || opened) {
    fl.resize(n);
    SCHK(T, hipMemcpyAsync(fl.data(), S->flags.d, n, hipMemcpyDeviceToHost, st));
  }
  SCHK(T, hipStreamSynchronize(st));
  if (closed)
    for (size_t i = 0; i < n; i++) closed[i] = (fl[i] & FLAG_CLOSED) ? 1 : 0;
  if (opened)
    for (size_t i = 0; i < n; i++) opened[i] = (fl[i] & FLAG_OPENED) ? 1 : 0;
  return MPLX_OK;
}

int space_edges(const Target &T, int width, int32_t n_q, const int32_t *qs, uint64_t cap, int32_t *child, int32_t *parent, int32_t *action) {
  Open O;
  if (int r = space_open(T, n_q, qs, O)) return r;
  const size_t n = (size_t)O.node_off[(size_t)n_q], ne = (size_t)O.edge_off[(size_t)n_q];
  if ((uint64_t)ne > cap) {
    char b[256];
    snprintf(b, sizeof(b), "state-space export: the listed queries hold %zu predecessor records, the caller's arrays hold %llu", ne, (unsigned long long)cap);
    return sfail(T, MPLX_ERR_CAPACITY, b);
  }
  if (n == 0 || ne == 0 || (!child && !parent && !action)) return MPLX_OK;
  mplx_space *S = nullptr;
  if (int r = space_nodes(T, O, width, S)) return r;  // (every query's records have been checked against its n_edges)
  hipStream_t st = O.C.stream;
  if (!S->have_edges) {
    SCHK(T, S->child.need(ne)); SCHK(T, S->parent.need(ne)); SCHK(T, S->action.need(ne));
    const uint32_t n_tiles = tiles_of(O);
    const SpaceQArgs A = space_args(O, *S, width, n_tiles);
    SCHK(T, hipEventRecord(S->ev0, st));
    hipLaunchKernelGGL(spaceq_edges_kernel, dim3(grid_for(n_tiles)), dim3(TILE), 0, st, A);
    SCHK(T, hipGetLastError());
    SCHK(T, hipEventRecord(S->ev1, st));
    unsigned long long back[2] = {0, 0};
    SCHK(T, hipMemcpyAsync(back, S->ctl.d, sizeof(back), hipMemcpyDeviceToHost, st));
    SCHK(T, hipStreamSynchronize(st));
    SCHK(T, hipEventElapsedTime(&S->ms[1], S->ev0, S->ev1));
    if ((uint32_t)back[1]) return space_err(T, *S, (uint32_t)back[1]);
    S->have_edges = true;
  }
  if (child) SCHK(T, hipMemcpyAsync(child, S->child.d, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, st));
  if (parent) SCHK(T, hipMemcpyAsync(parent, S->parent.d, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, st));
  if (action) SCHK(T, hipMemcpyAsync(action, S->action.d, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, st));
  SCHK(T, hipStreamSynchronize(st));
  return MPLX_OK;
}

int space_ms(mplx_ctx *ctx, float ms[2]) {
  mplx_space **slot = mplx_ctx_ext_space_slot(ctx);
  if (!slot || !ms) return MPLX_ERR_ARG;
  for (int k = 0; k < 2; k++) ms[k] = *slot ? (*slot)->ms[k] : 0.0f;
  return MPLX_OK;
}

Target voxel(mplx_ctx *ctx) { return Target{ctx, nullptr, false}; }
Target cloud(mplx_cloud *c) { return Target{mplx_cloud_internal_ctx(c), c, true}; }

}  // namespace

extern "C" int mplx_result_space_counts(mplx_ctx *ctx, int32_t n_q, const int32_t *qs, uint64_t *node_off, uint64_t *edge_off) {
  return space_counts(voxel(ctx), n_q, qs, node_off, edge_off);
}
extern "C" int mplx_result_space(mplx_ctx *ctx, int32_t n_q, const int32_t *qs, uint64_t cap_nodes, double *states, double *g, double *h, int32_t *closed,
                                 int32_t *opened) {
  return space_states(voxel(ctx), Row14::W, n_q, qs, cap_nodes, states, g, h, closed, opened);
}
extern "C" int mplx_result_space_edges(mplx_ctx *ctx, int32_t n_q, const int32_t *qs, uint64_t cap_edges, int32_t *child, int32_t *parent, int32_t *action) {
  return space_edges(voxel(ctx), Row14::W, n_q, qs, cap_edges, child, parent, action);
}
extern "C" int mplx_result_space_ms(const mplx_ctx *ctx, float ms[2]) { return space_ms(const_cast<mplx_ctx *>(ctx), ms); }

extern "C" int mplx_cloud_result_space_counts(mplx_cloud *c, int32_t n_q, const int32_t *qs, uint64_t *node_off, uint64_t *edge_off) {
  return space_counts(cloud(c), n_q, qs, node_off, edge_off);
}
extern "C" int mplx_cloud_result_space(mplx_cloud *c, int32_t n_q, const int32_t *qs, uint64_t cap_nodes, double *states, double *g, double *h, int32_t *closed,
                                       int32_t *opened) {
  return space_states(cloud(c), Row13::W, n_q, qs, cap_nodes, states, g, h, closed, opened);
}
extern "C" int mplx_cloud_result_space_edges(mplx_cloud *c, int32_t n_q, const int32_t *qs, uint64_t cap_edges, int32_t *child, int32_t *parent, int32_t *action) {
  return space_edges(cloud(c), Row13::W, n_q, qs, cap_edges, child, parent, action);
}
extern "C" int mplx_cloud_result_space_ms(const mplx_cloud *c, float ms[2]) { return space_ms(mplx_cloud_internal_ctx(const_cast<mplx_cloud *>(c)), ms); }
