// mplx_poly3_lpa.hip -- C-ABI mplx_plpa3_* (include/mplx.h): LPA* of the 3-D moving-obstacle planner -- PlannerBase::plan with
// setLPAstar(true), PolyMapPlanner<3>::updateNodes, getSubStateSpace.  mplx_plpa_* (mplx_poly_lpa.hip) one for one, on an mplx_poly3
// handle, states of 13 doubles (pos3 vel3 acc3 jrk3 t).  Kernels: mplx_poly3_lpa.h.  A translation unit of its own; what it needs of
// the mplx_poly3 handle comes through mplx_poly3_lpa_internal_view (mplx_poly3_lpa_host.h).  No CPU fallback: every compute entry
// launches a gfx950 kernel or fails.  The handle and the per-planner host steps are mplx_poly3_lpa_handle.h's, shared with the fleet
// entries (mplx_poly3_lpa_fleet.hip).
#include "../../include/mplx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mplx_poly3_lpa_handle.h"

using namespace mplx;

static std::string g_plpa3_create_error;

static int lf(mplx_plpa3 *l, int code, const char *fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (l) l->err = buf; else g_plpa3_create_error = buf;
  return code;
}
#define LH(l, x)                                                                                       \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess) return lf(l, MPLX_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_));      \
  } while (0)

template <bool GEN>
static void launch_plan(int control, hipStream_t s, const SearchParams &P, const PlpaArgs &A, const Poly3Dev &D) {
  if (control == CTRL_ACC) hipLaunchKernelGGL((plpa3_plan_kernel<CTRL_ACC, GEN>), dim3(1), dim3(64), 0, s, P, A, D);
  else hipLaunchKernelGGL((plpa3_plan_kernel<CTRL_JRK, GEN>), dim3(1), dim3(64), 0, s, P, A, D);
}
template <bool GEN>
static void launch_update(int control, int grid, hipStream_t s, const SearchParams &P, const PlpaArgs &A, const Poly3Dev &D) {
  if (control == CTRL_ACC) hipLaunchKernelGGL((plpa3_update_kernel<CTRL_ACC, GEN>), dim3(grid), dim3(64), 0, s, P, A, D);
  else hipLaunchKernelGGL((plpa3_update_kernel<CTRL_JRK, GEN>), dim3(grid), dim3(64), 0, s, P, A, D);
}

extern "C" int mplx_plpa3_create(mplx_poly3 *poly, mplx_plpa3 **out) {
  if (out) *out = nullptr;
  if (!poly || !out) return lf(nullptr, MPLX_ERR_ARG, "mplx_plpa3_create: %s", !poly ? "no mplx_poly3 handle (did mplx_poly3_create fail?)" : "out is NULL");
  mplx_plpa3 *l = new mplx_plpa3();
  l->poly = poly;
  *out = l;
  return MPLX_OK;
}
extern "C" void mplx_plpa3_destroy(mplx_plpa3 *l) {
  if (!l || l->in_fleet) return;  // (a fleet's member is the fleet's to destroy)
  plpa3_free(l);
  mplx_plpa_space_free(l->space);
  if (l->ev0) (void)hipEventDestroy(l->ev0);
  if (l->ev1) (void)hipEventDestroy(l->ev1);
  delete l;
}
extern "C" const char *mplx_plpa3_last_error(const mplx_plpa3 *l) { return l ? l->err.c_str() : g_plpa3_create_error.c_str(); }
extern "C" int mplx_plpa3_set_capacity(mplx_plpa3 *l, uint64_t max_nodes, uint64_t max_edges, uint64_t max_open_log) {
  if (!l) return MPLX_ERR_ARG;
  if (max_nodes) l->cap_nodes = max_nodes;
  if (max_edges) l->cap_edges = max_edges;
  if (max_open_log) l->cap_log = max_open_log;
  l->pools_valid = false;
  return MPLX_OK;
}
extern "C" int mplx_plpa3_initialized(const mplx_plpa3 *l) { return l && l->valid ? 1 : 0; }
extern "C" int mplx_plpa3_reset(mplx_plpa3 *l) {
  if (!l) return MPLX_ERR_ARG;
  l->valid = false;
  l->traj_len = 0;
  return MPLX_OK;
}

// the handle's view, refused before any launch: not configured / committed, VEL or SNP control, a world index out of range
static int plpa3_view(mplx_plpa3 *l, int32_t world, mplx_poly3_lpa_view &v) {
  const int r = plpa3_poly_view(l->poly, &l->err, v);
  if (r) return r;
  if (world < 0 || world >= v.n_worlds) return lf(l, MPLX_ERR_ARG, "world index out of range");
  plpa3_config_check(l, v);
  return MPLX_OK;
}

// PlannerBase::plan with setLPAstar(true): repairs and re-uses the state space of the previous plan when the goal and the start
// (= the current root) are unchanged; otherwise starts one.  start / goal: pos3 vel3 acc3 jrk3 t.
static int plpa3_plan_impl(mplx_plpa3 *l, int32_t world, const double *start, const double *goal, bool force_fresh, mplx_result *out) {
  mplx_poly3_lpa_view v;
  int r = plpa3_view(l, world, v);
  if (r) return r;
  LH(l, hipSetDevice(v.device));
  const int control = v.dev.control;
  if ((r = plpa3_ensure(l, control, v.dev.n_u)) != MPLX_OK) return r;
  if (!l->ev0) { LH(l, hipEventCreate(&l->ev0)); LH(l, hipEventCreate(&l->ev1)); }
  Plpa3Query q;
  plpa3_query(l, control, start, goal, force_fresh, q);
  const bool fresh = q.fresh;
  SearchParams P;
  plpa3_params(l, v, P);
  PlpaArgs A;
  plpa3_plan_args(l, v, world, fresh, A);
  hipStream_t s = v.stream;
  LH(l, hipMemcpyAsync(l->d_in, &q.in, sizeof(QueryIn), hipMemcpyHostToDevice, s));
  if (fresh) {
    LH(l, hipMemsetAsync(l->table, 0xFF, (size_t)l->table_slots * sizeof(unsigned long long), s));
    LH(l, hipMemsetAsync(l->d_st, 0, sizeof(LpaState), s));
  }
  LH(l, hipStreamSynchronize(s));  // (`q` is a local; the guard block is cleared with no copy in flight)
  if (v.guard) memset(v.guard, 0, sizeof(GuardBlock));
  const auto t0 = std::chrono::steady_clock::now();
  LH(l, hipEventRecord(l->ev0, s));
  if (v.general) launch_plan<true>(control, s, P, A, v.dev); else launch_plan<false>(control, s, P, A, v.dev);
  LH(l, hipGetLastError());
  LH(l, hipEventRecord(l->ev1, s));
  if ((r = plpa3_wait(&l->err, v, t0, "the 3-D moving-obstacle LPA* launch")) != MPLX_OK) {
    l->valid = false;
    l->traj_len = 0;
    return r;
  }
  LH(l, hipMemcpyAsync(&l->last_out, l->d_out, sizeof(QueryOut), hipMemcpyDeviceToHost, s));
  LH(l, hipMemcpyAsync(&l->st, l->d_st, sizeof(LpaState), hipMemcpyDeviceToHost, s));
  LH(l, hipStreamSynchronize(s));
  LH(l, hipEventElapsedTime(&l->last_ms, l->ev0, l->ev1));
  return plpa3_plan_finish(l, q, v.cfg_epoch, goal, out, nullptr);
}
extern "C" int mplx_plpa3_plan(mplx_plpa3 *l, int32_t world, const double *start, const double *goal, double eps, double tol_pos, double tol_vel, int32_t max_expand,
                               int32_t heur_ignore_dynamics, mplx_result *out) {
  if (!l || !start || !goal || !out) return lf(l, MPLX_ERR_ARG, "null argument");
  plpa3_setup(l, eps, tol_pos, tol_vel, max_expand, heur_ignore_dynamics);
  return plpa3_plan_impl(l, world, start, goal, false, out);
}

// PolyMapPlanner<3>::updateNodes (poly_map_planner.h:61-93), after the world's obstacles / start time were committed again
extern "C" int mplx_plpa3_update_nodes(mplx_plpa3 *l, int32_t world, uint64_t *n_blocked, uint64_t *n_cleared) {
  if (!l) return MPLX_ERR_ARG;
  if (n_blocked) *n_blocked = 0;
  if (n_cleared) *n_cleared = 0;
  l->changed.clear();
  mplx_poly3_lpa_view v;
  int r = plpa3_view(l, world, v);
  if (r) return r;
  if (!l->valid) return MPLX_OK;  // (updateNodes returns at once without a state space: poly_map_planner.h:65)
  if (!l->pools_valid || l->pool_control != v.dev.control || l->succ_n_u != v.dev.n_u) return lf(l, MPLX_ERR_ARG, "the planner set-up changed since the state space was built");
  LH(l, hipSetDevice(v.device));
  SearchParams P;
  plpa3_params(l, v, P);
  PlpaArgs A;
  plpa3_update_args(l, world, P, A);
  hipStream_t s = v.stream;
  LH(l, hipMemsetAsync(l->d_counters, 0, sizeof(uint32_t) * 4, s));
  const int grid = plpa3_update_grid(l);
  if (v.general) launch_update<true>(v.dev.control, grid, s, P, A, v.dev); else launch_update<false>(v.dev.control, grid, s, P, A, v.dev);
  LH(l, hipGetLastError());
  uint32_t ctr[4] = {0, 0, 0, 0};
  LH(l, hipMemcpyAsync(ctr, l->d_counters, sizeof(ctr), hipMemcpyDeviceToHost, s));
  LH(l, hipStreamSynchronize(s));
  return plpa3_update_finish(l, ctr, A.changed_cap, v.commit_epoch, n_blocked, n_cleared, nullptr);
}
// the entries updateNodes changed, by entry number (entry -> parent state and action: mplx_plpa3_result_entries / _nodes)
extern "C" int mplx_plpa3_changed(mplx_plpa3 *l, uint64_t cap, int32_t *entry, int32_t *now_blocked, uint64_t *n) {
  if (!l || !n) return MPLX_ERR_ARG;
  *n = l->changed.size();
  for (size_t i = 0; i < l->changed.size() && i < cap; i++) {
    if (entry) entry[i] = (int32_t)(l->changed[i] & 0x7FFFFFFFu);
    if (now_blocked) now_blocked[i] = (int32_t)(l->changed[i] >> 31);
  }
  return MPLX_OK;
}
// PlannerBase::getSubStateSpace(time_step): by planning afresh from the time_step-th state of the last trajectory to the planner's
// goal; the stored trajectory is dropped (the caller plans from its state next)
extern "C" int mplx_plpa3_sub_state_space(mplx_plpa3 *l, int32_t world, int32_t time_step) {
  if (!l) return MPLX_ERR_ARG;
  if (!l->valid || l->traj_len <= 0) return MPLX_OK;
  if (time_step < 0 || time_step > l->traj_len) return lf(l, MPLX_ERR_ARG, "time_step %d outside the last trajectory (%d primitives)", time_step, l->traj_len);
  double start[13], goal[13];
  memcpy(start, &l->traj_states[(size_t)(l->traj_len - time_step) * 13], sizeof(start));  // (device order is goal -> start)
  for (int i = 0; i < 13; i++) goal[i] = l->goal[i];
  mplx_result res;
  const int r = plpa3_plan_impl(l, world, start, goal, true, &res);
  l->traj_len = 0;
  return r;
}
extern "C" int mplx_plpa3_traj_len(const mplx_plpa3 *l) { return l ? l->traj_len : 0; }
// trajectory of the last successful plan, start -> goal: actions[len], node_ids[len + 1], states (len + 1) x 13
extern "C" int mplx_plpa3_result_traj(mplx_plpa3 *l, int32_t *actions, int32_t *node_ids, double *states) {
  if (!l) return MPLX_ERR_ARG;
  const int len = l->traj_len;
  for (int i = 0; i <= len && len > 0; i++) {
    if (node_ids) node_ids[i] = l->traj_nodes[(size_t)(len - i)];
    if (states) memcpy(states + 13 * (size_t)i, &l->traj_states[(size_t)(len - i) * 13], sizeof(double) * 13);
  }
  for (int i = 0; i < len; i++)
    if (actions) actions[i] = l->traj_actions[(size_t)(len - 1 - i)];
  return MPLX_OK;
}
extern "C" int mplx_plpa3_last_kernel_ms(const mplx_plpa3 *l, float *ms) {
  if (!l || !ms) return MPLX_ERR_ARG;
  *ms = l->last_ms;
  return MPLX_OK;
}
extern "C" int mplx_plpa3_counts(const mplx_plpa3 *l, uint64_t *n_nodes, uint64_t *n_entries) {
  if (!l) return MPLX_ERR_ARG;
  if (n_nodes) *n_nodes = l->valid ? l->st.n_nodes : 0;
  if (n_entries) *n_entries = l->valid ? l->st.n_edges : 0;
  return MPLX_OK;
}
extern "C" int mplx_plpa3_result_expanded(mplx_plpa3 *l, uint32_t cap, int32_t *ids, uint32_t *n) {
  if (!l || !ids || !n) return MPLX_ERR_ARG;
  const uint32_t cnt = std::min(l->last_out.n_recorded, cap);
  if (cnt) LH(l, hipMemcpy(ids, l->d_rec, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
  *n = cnt;
  return MPLX_OK;
}
// state-space dump: per state pos3 vel3 acc3 jrk3 t | g rhs h | closed opened built; arrays of `cap` states
extern "C" int mplx_plpa3_result_nodes(mplx_plpa3 *l, uint64_t cap, double *states, double *g, double *rhs, double *h, int32_t *closed, int32_t *opened, int32_t *built) {
  if (!l) return MPLX_ERR_ARG;
  if (!l->valid) return MPLX_OK;
  const size_t n = l->st.n_nodes;
  if ((uint64_t)n > cap) return lf(l, MPLX_ERR_CAPACITY, "state-space dump: %zu states, the caller's arrays hold %llu", n, (unsigned long long)cap);
  const int control = l->pool_control, ns = state_len(control), rb = rec_bytes(control), hot = rec_hot_bytes(control);
  std::vector<char> buf(n * (size_t)rb);
  LH(l, hipMemcpy(buf.data(), l->node_pool, buf.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) {
    const char *r = buf.data() + i * rb;
    const double *st = (const double *)(r + hot);
    if (states) {
      double *o = states + 13 * i;
      for (int k = 0; k < 12; k++) o[k] = k < ns ? st[k] : 0.0;
      o[12] = st[ns];
    }
    const uint32_t fl = *(const uint32_t *)(r + 16);
    if (g) g[i] = *(const double *)r;
    if (h) h[i] = *(const double *)(r + 8);
    if (rhs) rhs[i] = st[ns + 1];
    if (closed) closed[i] = (fl & FLAG_CLOSED) ? 1 : 0;
    if (opened) opened[i] = (fl & FLAG_OPENED) ? 1 : 0;
    if (built) built[i] = (fl & FLAG_BUILT) ? 1 : 0;
  }
  return MPLX_OK;
}
// predecessor entries in creation order: child, parent, action, blocked; arrays of `cap` entries
extern "C" int mplx_plpa3_result_entries(mplx_plpa3 *l, uint64_t cap, int32_t *child, int32_t *parent, int32_t *action, int32_t *blocked) {
  if (!l) return MPLX_ERR_ARG;
  if (!l->valid) return MPLX_OK;
  const size_t n = l->st.n_nodes, ne = l->st.n_edges;
  if ((uint64_t)ne > cap) return lf(l, MPLX_ERR_CAPACITY, "entry dump: %zu entries, the caller's arrays hold %llu", ne, (unsigned long long)cap);
  const int rb = rec_bytes(l->pool_control);
  std::vector<char> nb(n * (size_t)rb);
  std::vector<EdgeRec> eb(ne);
  LH(l, hipMemcpy(nb.data(), l->node_pool, nb.size(), hipMemcpyDeviceToHost));
  if (ne) LH(l, hipMemcpy(eb.data(), l->edge_pool, sizeof(EdgeRec) * ne, hipMemcpyDeviceToHost));
  for (size_t e = 0; e < ne; e++) {
    if (parent) parent[e] = (int32_t)eb[e].parent;
    if (action) action[e] = (int32_t)(eb[e].action & ~EDGE_BLOCKED);
    if (blocked) blocked[e] = (eb[e].action & EDGE_BLOCKED) ? 1 : 0;
  }
  if (child)
    for (size_t i = 0; i < n; i++)
      for (uint32_t e = *(const uint32_t *)(nb.data() + i * rb + 20); e != NIL && e < ne; e = eb[e].next) child[e] = (int32_t)i;
  return MPLX_OK;
}
