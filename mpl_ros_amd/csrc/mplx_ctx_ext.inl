// mplx_ctx_ext.inl -- (internal) what a search kernel of another translation unit needs of a planner context: its pools,
// batch buffers, launch guard and result getters.  Included by mplx_api.hip; host code only.  Used by the point-cloud
// planner (mplx_cloud.hip), whose kernels are instantiated in that unit (mplx_api.hip takes minutes to compile).
#include "mplx_ctx_ext.h"

// One search launch of n queries on the context (configured by mplx_planner_config): the pools are sized for
// min(n, n_slots) workgroups, the queries uploaded in order, `launch` starts the kernel on the context's stream with the
// SearchParams filled here, and the wait goes through the launch guard.  Afterwards the context's result getters
// (mplx_result_traj / _expanded, mplx_ctx_ext_nodes) answer for this batch.
int mplx_ctx_ext_plan(mplx_ctx *c, int n, const mplx::QueryIn *in, mplx_ext_launch launch, void *user, const char *what, mplx_result *out) {
  if (!c || n <= 0 || !in || !launch || !out) return fail(c, MPLX_ERR_ARG, "bad argument");
  MPLX_REFUSE_PENDING(c);
  if (!c->have_cfg) return fail(c, MPLX_ERR_ARG, "planner not configured");
  if (c->wedged) return fail(c, MPLX_ERR_TIMEOUT, "this context was lost to a launch that never ended (destroy it)");
  if (n >= 0xFFFF) return fail(c, MPLX_ERR_ARG, "at most 65534 queries per batch");
  HIPCHK(c, hipSetDevice(c->device));
  const int helpers_saved = c->helpers;
  c->helpers = 0;  // (no look-ahead cache arrays for these kernels)
  const int slots = n < c->n_slots ? n : c->n_slots;
  int r = ensure_pools(c, slots);
  c->helpers = helpers_saved;
  if (r != MPLX_OK) return r;
  if ((r = ensure_batch(c, n)) != MPLX_OK) return r;
  std::vector<int32_t> order((size_t)n);
  for (int k = 0; k < n; k++) order[(size_t)k] = k;
  SearchParams P = c->pools;
  fill_params(c, P);
  P.boxes = nullptr;
  P.xflags = 0;
  P.cap_rec = c->cap_rec;
  P.nq = n;
  P.queries = c->d_in;
  P.order = c->d_order;
  P.out = c->d_out;
  P.traj_nodes = c->d_traj_nodes; P.traj_actions = c->d_traj_actions; P.traj_states = c->d_traj_states;
  P.traj_yaw = nullptr;
  P.rec_ids = c->cap_rec ? c->d_rec : nullptr;
  P.node_tables = c->d_node_tables;
  P.edge_tables = c->d_edge_tables;
  P.next_query = c->d_next;
  P.help_lead = slots;
  P.help_max = 0;
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(c->d_order, order.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
  if (int rt = table_prepare(c, P, st)) return rt;
  HIPCHK(c, hipMemsetAsync(P.chunk_next, 0, 4 * sizeof(uint32_t), st));
  P.chunk_bits = nullptr;
  HIPCHK(c, hipMemcpyAsync(c->d_in, in, sizeof(QueryIn) * (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(c->d_next, 0, sizeof(int32_t), st));
  guard_arm(c);
  HIPCHK(c, hipEventRecord(c->ev0, st));
  if (!launch(user, slots, st, P)) return fail(c, MPLX_ERR_ARG, "no build of %s for this configuration", what);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev1, st));
  c->last_out.resize((size_t)n);
  if (int rw = guard_wait(c, st, what)) {
    c->last_nq = 0;
    return rw;
  }
  HIPCHK(c, hipMemcpyAsync(c->last_out.data(), c->d_out, sizeof(QueryOut) * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  for (int k = 0; k < n; k++) fill_result(c->last_out[(size_t)k], out[k]);
  c->last_nq = n;
  c->last_single = (n == 1);
  c->last_control = c->cfg.control;
  c->last_yaw = false;
  c->last_dt = c->cfg.dt;
  c->last_U = c->U;
  c->plan_epoch++;
  return MPLX_OK;
}

// The state space of query q of the last batch: n_nodes states in id order, g, closed / opened flags (mplx_result_nodes for
// any query of a batch)
int mplx_ctx_ext_nodes(mplx_ctx *c, int q, uint64_t cap, mplx_waypoint *coords, double *g, int32_t *closed, int32_t *opened) {
  if (!c || q < 0 || q >= c->last_nq || !c->pools_valid) return fail(c, MPLX_ERR_ARG, "no such query");
  MPLX_REFUSE_PENDING(c);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = c->last_out[(size_t)q].n_nodes;
  if (n == 0) return MPLX_OK;
  if ((uint64_t)n > cap) return fail(c, MPLX_ERR_CAPACITY, "state-space dump: query %d created %zu states, the caller's arrays hold %llu", q, n, (unsigned long long)cap);
  const int control = c->pool_control, nk = state_len(control), rb = rec_bytes(control), hot = rec_hot_bytes(control);
  std::vector<uint32_t> tbl(MAX_NODE_CH);
  HIPCHK(c, hipMemcpyAsync(tbl.data(), c->d_node_tables + (size_t)q * MAX_NODE_CH, sizeof(uint32_t) * MAX_NODE_CH, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t per = (size_t)1 << NODE_CH_LOG;
  std::vector<char> buf(per * rb);
  for (size_t base = 0; base < n; base += per) {
    const size_t cnt = n - base < per ? n - base : per;
    const uint32_t ch = tbl[base >> NODE_CH_LOG];
    if (ch == NIL) return fail(c, MPLX_ERR_ARG, "inconsistent chunk table");
    HIPCHK(c, hipMemcpyAsync(buf.data(), c->pools.node_pool + ((size_t)ch << NODE_CH_LOG) * rb, cnt * rb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < cnt; k++) {
      const char *r = buf.data() + k * rb;
      const size_t i = base + k;
      uint32_t fl;
      memcpy(&fl, r + 16, 4);
      if (g) memcpy(&g[i], r, 8);
      if (closed) closed[i] = (fl & FLAG_CLOSED) ? 1 : 0;
      if (opened) opened[i] = (fl & FLAG_OPENED) ? 1 : 0;
      if (coords) {
        mplx_waypoint &w = coords[i];
        memset(&w, 0, sizeof(w));
        const double *st = (const double *)(r + hot);
        for (int d = 0; d < nk; d++) {
          double *dst = d < 3 ? w.pos : d < 6 ? w.vel : d < 9 ? w.acc : w.jrk;
          dst[d % 3] = st[d];
        }
        w.t = st[nk];
        w.control = control;
      }
    }
  }
  return MPLX_OK;
}
const char *mplx_ctx_ext_error(const mplx_ctx *c) { return c ? c->err.c_str() : ""; }

// (mplx_ctx_ext_view) the last batch's pools, tables and outcomes for an export that runs in another translation unit
int mplx_ctx_ext_view_get(const mplx_ctx *c, mplx_ctx_ext_view *out) {
  if (!c || !out) return MPLX_ERR_ARG;
  out->device = c->device;
  out->stream = c->stream;
  out->last_nq = c->last_nq;
  out->pending = c->pending ? 1 : 0;
  out->pools_valid = c->pools_valid ? 1 : 0;
  out->recycled = c->last_recycled ? 1 : 0;
  out->pool_control = c->pool_control;
  out->last_yaw = c->last_yaw ? 1 : 0;
  out->last_out = c->last_out.data();
  out->node_pool = c->pools.node_pool; out->edge_pool = c->pools.edge_pool;
  out->node_chunks = c->pools.node_chunks; out->edge_chunks = c->pools.edge_chunks;
  out->node_tables = c->d_node_tables; out->edge_tables = c->d_edge_tables;
  out->plan_epoch = c->plan_epoch;
  out->guard = c->guard;
  out->deadline_s = c->deadline_s;
  return MPLX_OK;
}
mplx_space **mplx_ctx_ext_space_slot(mplx_ctx *c) { return c ? &c->space : nullptr; }
int mplx_ctx_ext_fail(mplx_ctx *c, int code, const char *msg) { return fail(c, code, "%s", msg); }
