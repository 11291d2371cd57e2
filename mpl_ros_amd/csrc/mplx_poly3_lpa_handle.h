// mplx_poly3_lpa_handle.h -- the mplx_plpa3 handle and the per-planner host steps of its calls, which the single-planner entries
// (mplx_poly3_lpa.hip) and the fleet entries (mplx_poly3_lpa_fleet.hip) share: set-up, pool allocation, the fresh-or-repair decision and
// the query, the per-handle kernel arguments, what is done with the results of a plan launch (status, trajectory copy, validity,
// epochs) and of an updateNodes launch (counters, changed list, epoch), the wait with the deadline.  As mplx_poly_lpa_handle.h is for
// the 2-D planner.  Host only; the functions are defined here (inline), so that both units decide and book a planner through the
// same code.
#pragma once
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mplx.h"
#include "mplx_poly3_lpa.h"
#include "mplx_poly3_lpa_host.h"
#include "mplx_plpa_space.h"

struct mplx_plpa3 {
  mplx_poly3 *poly = nullptr;
  std::string err;
  // capacities and pools (flat, private to the handle: chunk tables are the identity)
  uint64_t cap_nodes = 1 << 18, cap_edges = 1 << 21, cap_log = 1 << 21;
  bool pools_valid = false;
  int pool_control = 0;
  char *node_pool = nullptr, *edge_pool = nullptr, *open_pool = nullptr;
  unsigned long long *table = nullptr;
  uint64_t table_slots = 0;
  uint32_t *bkt_head = nullptr;
  mplx::LpaState *d_st = nullptr;
  mplx::QueryIn *d_in = nullptr;
  mplx::QueryOut *d_out = nullptr;
  int32_t *d_traj_nodes = nullptr, *d_traj_actions = nullptr, *d_rec = nullptr;
  double *d_traj_states = nullptr;
  uint32_t *d_changed = nullptr, *d_counters = nullptr;
  double *d_edge_cost = nullptr;
  uint32_t *d_succ_child = nullptr, *d_succ_entry = nullptr;  // per state x control input (null when that would be too large)
  int succ_n_u = 0;
  uint64_t synced_epoch = ~0ull;  // mplx_poly3 commit count the entries' blocked bits were last brought in step with
  uint64_t cfg_epoch = ~0ull;     // mplx_poly3 config count the space was built under
  uint32_t cap_rec = 0;
  // a member of a fleet: d_st / d_in / d_out / d_counters are these slices of the fleet's arrays (not the handle's to free)
  mplx::LpaState *fleet_st = nullptr;
  mplx::QueryIn *fleet_in = nullptr;
  mplx::QueryOut *fleet_out = nullptr;
  uint32_t *fleet_counters = nullptr;
  bool in_fleet = false;  // owned by a fleet: mplx_plpa3_destroy ignores it
  // host copies
  mplx::LpaState st{};
  mplx::QueryOut last_out{};
  bool valid = false;
  double goal[13] = {0}, eps = 1.0, tol_pos = 0.5, tol_vel = -1.0;
  int32_t max_expand = -1, heur_ignore_dynamics = 1;
  int32_t root_key[mplx::MAX_KEY + 1] = {0};
  int traj_len = 0;
  std::vector<int32_t> traj_nodes, traj_actions;
  std::vector<double> traj_states;
  std::vector<uint32_t> changed;
  float last_ms = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  mplx_plpa_space *space = nullptr;  // scratch of the state-space exports (mplx_plpa_space.hip)
};

// the query of one plan() and the decision it starts with
struct Plpa3Query {
  mplx::QueryIn in;
  int32_t key[mplx::MAX_KEY + 1];  // of the start state (time-keyed)
  bool fresh;                      // a new state space is started (else the one of the last plan is repaired)
};

inline int plpa3_fail(std::string *err, int code, const char *fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return code;
}
#define PLPA3_H(l, x)                                                                                              \
  do {                                                                                                             \
    hipError_t e_ = (x);                                                                                           \
    if (e_ != hipSuccess) return plpa3_fail(&(l)->err, MPLX_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_));  \
  } while (0)

inline uint64_t plpa3_chunks_of(uint64_t cap, int log2) { return std::max<uint64_t>(1, (cap + (1u << log2) - 1) >> log2); }

// the planner set-up of a plan() call; a space that was built under another eps / tolerance / heuristic mode is given up
inline void plpa3_setup(mplx_plpa3 *l, double eps, double tol_pos, double tol_vel, int32_t max_expand, int32_t heur_ignore_dynamics) {
  if (l->valid && (l->eps != eps || l->tol_pos != tol_pos || l->tol_vel != tol_vel || l->heur_ignore_dynamics != heur_ignore_dynamics)) l->valid = false;
  l->eps = eps; l->tol_pos = tol_pos; l->tol_vel = tol_vel; l->max_expand = max_expand; l->heur_ignore_dynamics = heur_ignore_dynamics;
}

inline void plpa3_free(mplx_plpa3 *l) {
  using namespace mplx;
  (void)hipFree(l->node_pool); (void)hipFree(l->edge_pool); (void)hipFree(l->open_pool); (void)hipFree(l->table); (void)hipFree(l->bkt_head);
  if (!l->fleet_st) { (void)hipFree(l->d_st); (void)hipFree(l->d_in); (void)hipFree(l->d_out); (void)hipFree(l->d_counters); }
  (void)hipFree(l->d_traj_nodes); (void)hipFree(l->d_traj_actions);
  (void)hipFree(l->d_traj_states); (void)hipFree(l->d_changed); (void)hipFree(l->d_rec); (void)hipFree(l->d_edge_cost); (void)hipFree(l->d_succ_child); (void)hipFree(l->d_succ_entry);
  l->d_edge_cost = nullptr; l->d_succ_child = l->d_succ_entry = nullptr;
  l->node_pool = l->edge_pool = l->open_pool = nullptr;
  l->table = nullptr; l->bkt_head = nullptr; l->d_st = nullptr; l->d_in = nullptr; l->d_out = nullptr;
  l->d_traj_nodes = l->d_traj_actions = l->d_rec = nullptr; l->d_traj_states = nullptr; l->d_changed = l->d_counters = nullptr;
  l->pools_valid = false;
}
// pools for this control kind and lattice width (allocated on the first call and after mplx_plpa3_set_capacity)
inline int plpa3_ensure(mplx_plpa3 *l, int control, int n_u) {
  using namespace mplx;
  if (l->pools_valid && l->pool_control == control && l->succ_n_u == n_u) return MPLX_OK;
  plpa3_free(l);
  l->valid = false;
  const uint64_t nch = plpa3_chunks_of(l->cap_nodes, NODE_CH_LOG), ech = plpa3_chunks_of(l->cap_edges, EDGE_CH_LOG), och = plpa3_chunks_of(l->cap_log, OPEN_CH_LOG);
  if (nch > (uint64_t)MAX_NODE_CH || ech > (uint64_t)MAX_EDGE_CH || och > (uint64_t)MAX_OPEN_CH)
    return plpa3_fail(&l->err, MPLX_ERR_ARG, "capacity too large (at most %d node / %d predecessor / %d OPEN-log chunks)", MAX_NODE_CH, MAX_EDGE_CH, MAX_OPEN_CH);
  uint64_t slots = 1;
  while (slots < 4ull * (nch << NODE_CH_LOG)) slots <<= 1;
  l->table_slots = slots;
  PLPA3_H(l, hipMalloc((void **)&l->node_pool, (size_t)(nch << NODE_CH_LOG) * rec_bytes(control)));
  PLPA3_H(l, hipMalloc((void **)&l->edge_pool, (size_t)(ech << EDGE_CH_LOG) * EDGE_BYTES));
  PLPA3_H(l, hipMalloc((void **)&l->open_pool, (size_t)(och << OPEN_CH_LOG) * OPEN_BYTES));
  PLPA3_H(l, hipMalloc((void **)&l->table, (size_t)l->table_slots * sizeof(unsigned long long)));
  PLPA3_H(l, hipMalloc((void **)&l->bkt_head, sizeof(uint32_t) * 2 * NB * NSUB));
  PLPA3_H(l, hipMemset(l->bkt_head, 0xFF, sizeof(uint32_t) * 2 * NB * NSUB));
  if (l->fleet_st) {
    l->d_st = l->fleet_st; l->d_in = l->fleet_in; l->d_out = l->fleet_out; l->d_counters = l->fleet_counters;
  } else {
    PLPA3_H(l, hipMalloc((void **)&l->d_st, sizeof(LpaState)));
    PLPA3_H(l, hipMalloc((void **)&l->d_in, sizeof(QueryIn)));
    PLPA3_H(l, hipMalloc((void **)&l->d_out, sizeof(QueryOut)));
    PLPA3_H(l, hipMalloc((void **)&l->d_counters, sizeof(uint32_t) * 4));
  }
  PLPA3_H(l, hipMalloc((void **)&l->d_traj_nodes, sizeof(int32_t) * (MAX_TRAJ + 1)));
  PLPA3_H(l, hipMalloc((void **)&l->d_traj_actions, sizeof(int32_t) * MAX_TRAJ));
  PLPA3_H(l, hipMalloc((void **)&l->d_traj_states, sizeof(double) * (MAX_TRAJ + 1) * 13));
  PLPA3_H(l, hipMalloc((void **)&l->d_changed, sizeof(uint32_t) * (size_t)(ech << EDGE_CH_LOG)));
  PLPA3_H(l, hipMalloc((void **)&l->d_edge_cost, sizeof(double) * (size_t)(ech << EDGE_CH_LOG)));
  l->succ_n_u = n_u;
  if ((nch << NODE_CH_LOG) * (uint64_t)n_u * 8ull <= (4ull << 30)) {  // (beyond 4 GB the re-expansion shortcut is off: get_succ runs again)
    PLPA3_H(l, hipMalloc((void **)&l->d_succ_child, sizeof(uint32_t) * (size_t)(nch << NODE_CH_LOG) * (size_t)n_u));
    PLPA3_H(l, hipMalloc((void **)&l->d_succ_entry, sizeof(uint32_t) * (size_t)(nch << NODE_CH_LOG) * (size_t)n_u));
  }
  l->cap_rec = (uint32_t)std::min<uint64_t>(l->cap_nodes, 1u << 24);
  PLPA3_H(l, hipMalloc((void **)&l->d_rec, sizeof(int32_t) * (size_t)l->cap_rec));
  l->pool_control = control;
  l->pools_valid = true;
  return MPLX_OK;
}

// the poly handle's view, refused before any launch: not configured / committed, VEL or SNP control, too many control inputs
inline int plpa3_poly_view(mplx_poly3 *poly, std::string *err, mplx_poly3_lpa_view &v) {
  using namespace mplx;
  const int r = mplx_poly3_lpa_internal_view(poly, &v);
  if (r != MPLX_OK) return plpa3_fail(err, r, "%s", mplx_poly3_last_error(poly));
  if (v.dev.control != CTRL_ACC && v.dev.control != CTRL_JRK)
    return plpa3_fail(err, MPLX_ERR_ARG, "the moving-obstacle LPA* runs ACC or JRK states (time-keyed: an SNP state's key would need 13 integers; VEL states have no caller)");
  if (v.dev.n_u > POLY3_MAX_U) return plpa3_fail(err, MPLX_ERR_ARG, "at most %d control inputs", POLY3_MAX_U);
  return MPLX_OK;
}
// mplx_poly3_config since the space was built: it is dropped
inline void plpa3_config_check(mplx_plpa3 *l, const mplx_poly3_lpa_view &v) {
  if (l->valid && l->cfg_epoch != v.cfg_epoch) {
    l->valid = false;
    l->traj_len = 0;
  }
}

inline void plpa3_key_of(int control, const double *s13, int32_t *key) {
  using namespace mplx;
  State st{};
  for (int a = 0; a < 3; a++) {
    st.p[a] = s13[a]; st.v[a] = s13[3 + a];
    if (control == CTRL_JRK) st.a[a] = s13[6 + a];
  }
  const int n = state_key(control, st, key);
  key[n] = (int32_t)round(s13[12] / 0.1);
}
// the space of the last plan is repaired when it is valid, the goal is the same and the start is its root.  start / goal: pos3 vel3 acc3 jrk3 t.
inline void plpa3_query(const mplx_plpa3 *l, int control, const double *start, const double *goal, bool force_fresh, Plpa3Query &q) {
  using namespace mplx;
  QueryIn &in = q.in;
  in = QueryIn{};
  for (int a = 0; a < 3; a++) {
    in.start.p[a] = start[a]; in.start.v[a] = start[3 + a];
    in.goal.p[a] = goal[a]; in.goal.v[a] = goal[3 + a];
    if (control == CTRL_JRK) { in.start.a[a] = start[6 + a]; in.goal.a[a] = goal[6 + a]; }
  }
  in.start_t = start[12];
  in.goal_control = control;
  memset(q.key, 0, sizeof(q.key));
  plpa3_key_of(control, start, q.key);
  bool same_goal = true;
  for (int i = 0; i < 12; i++) same_goal = same_goal && l->goal[i] == goal[i];
  q.fresh = force_fresh || !l->valid || !same_goal || memcmp(q.key, l->root_key, sizeof(q.key)) != 0;
}
inline void plpa3_params(const mplx_plpa3 *l, const mplx_poly3_lpa_view &v, mplx::SearchParams &P) {
  using namespace mplx;
  P = SearchParams{};
  P.control = v.dev.control; P.n_u = v.dev.n_u;
  P.ns = state_len(v.dev.control); P.nk = state_len(v.dev.control);
  P.dt = v.dev.dt; P.v_max = v.dev.v_max; P.a_max = v.dev.a_max; P.j_max = v.dev.j_max; P.w = v.dev.w;
  P.eps = l->eps; P.tol_pos = l->tol_pos; P.tol_vel = l->tol_vel; P.tol_acc = -1.0; P.t_max = INFINITY;
  P.max_expand = l->max_expand; P.heur_ignore_dynamics = l->heur_ignore_dynamics;
  P.bucket_width = P.w * P.dt > 0 ? P.w * P.dt * 8.0 : 1.0;  // (coarse OPEN bucket; a fine one is 1 / 1024 of it: the 2-D planner's choice)
  P.node_pool = l->node_pool; P.edge_pool = l->edge_pool; P.open_pool = l->open_pool;
  P.node_chunks = (uint32_t)plpa3_chunks_of(l->cap_nodes, NODE_CH_LOG);
  P.edge_chunks = (uint32_t)plpa3_chunks_of(l->cap_edges, EDGE_CH_LOG);
  P.open_chunks = (uint32_t)plpa3_chunks_of(l->cap_log, OPEN_CH_LOG);
  P.table = l->table; P.table_mask = l->table_slots - 1;
  P.bkt_head = l->bkt_head;
  P.cap_rec = l->cap_rec;
  P.nq = 1;
  P.queries = l->d_in; P.out = l->d_out;
  P.traj_nodes = l->d_traj_nodes; P.traj_actions = l->d_traj_actions; P.traj_states = l->d_traj_states;
  P.rec_ids = l->d_rec;
  P.guard = v.guard;
}
// PlpaArgs of a plan launch; a fresh space is in step with the world as committed now (synced_epoch)
inline void plpa3_plan_args(mplx_plpa3 *l, const mplx_poly3_lpa_view &v, int32_t world, bool fresh, mplx::PlpaArgs &A) {
  A = mplx::PlpaArgs{};
  A.st = l->d_st; A.fresh = fresh ? 1 : 0; A.world = world; A.edge_cost = l->d_edge_cost;
  A.succ_child = l->d_succ_child; A.succ_entry = l->d_succ_entry;
  // the entries are in step with the committed world when the space is new, or when updateNodes ran after the last commit
  if (fresh) l->synced_epoch = v.commit_epoch;
  A.trust_entries = (l->synced_epoch == v.commit_epoch && getenv("MPLX_PLPA_NO_REUSE") == nullptr) ? 1 : 0;
}
// after a plan launch, l->last_out and l->st hold the results: fills `out`, keeps or drops the space (cfg_epoch: the mplx_poly3 config
// count of the launch), fetches the trajectory (s != nullptr: with asynchronous copies on s, which the caller waits for)
inline int plpa3_plan_finish(mplx_plpa3 *l, const Plpa3Query &q, uint64_t cfg_epoch, const double *goal, mplx_result *out, hipStream_t s) {
  using namespace mplx;
  const QueryOut &o = l->last_out;
  if (out) {
    memset(out, 0, sizeof(*out));
    out->status = o.status; out->traj_len = o.traj_len; out->cost = o.cost;
    out->n_expanded = o.n_expanded; out->n_closed = o.n_closed; out->n_nodes = o.n_nodes; out->n_edges = o.n_edges;
    out->n_primitives = o.n_primitives; out->n_succ = o.n_succ; out->n_succ_finite = o.n_succ_finite;
    out->n_push = o.n_push; out->n_refill = query_refills(o); out->n_evict = o.n_evict; out->expand_hash = o.expand_hash;
  }
  l->traj_len = 0;
  if (o.status == MPLX_PLAN_POOL_FULL || o.status == MPLX_PLAN_INTERNAL || o.status == MPLX_PLAN_ABORTED) {
    l->valid = false;
    // (as mplx_poly3_plan_batch: the same code, and the state space is dropped)
    if (o.status == MPLX_PLAN_INTERNAL) return plpa3_fail(&l->err, MPLX_ERR_ARG, "internal: a hyperplane equation of degree > 2 was met by the quadratic-only kernel");
  } else if (l->st.valid) {
    l->valid = true;
    l->cfg_epoch = cfg_epoch;
    for (int i = 0; i < 13; i++) l->goal[i] = goal[i];
    if (q.fresh) memcpy(l->root_key, q.key, sizeof(q.key));
  } else if (q.fresh) {
    l->valid = false;  // (the start already satisfies the goal, or lies outside the map: no state space was built)
    for (int i = 0; i < 13; i++) l->goal[i] = goal[i];
  }
  if (o.status == MPLX_PLAN_OK && o.traj_len > 0) {
    const int len = o.traj_len;
    l->traj_len = len;
    l->traj_nodes.assign((size_t)len + 1, 0);
    l->traj_actions.assign((size_t)len, 0);
    l->traj_states.assign((size_t)(len + 1) * 13, 0.0);
    if (s) {
      PLPA3_H(l, hipMemcpyAsync(l->traj_nodes.data(), l->d_traj_nodes, sizeof(int32_t) * (size_t)(len + 1), hipMemcpyDeviceToHost, s));
      PLPA3_H(l, hipMemcpyAsync(l->traj_actions.data(), l->d_traj_actions, sizeof(int32_t) * (size_t)len, hipMemcpyDeviceToHost, s));
      PLPA3_H(l, hipMemcpyAsync(l->traj_states.data(), l->d_traj_states, sizeof(double) * (size_t)(len + 1) * 13, hipMemcpyDeviceToHost, s));
    } else {
      PLPA3_H(l, hipMemcpy(l->traj_nodes.data(), l->d_traj_nodes, sizeof(int32_t) * (size_t)(len + 1), hipMemcpyDeviceToHost));
      PLPA3_H(l, hipMemcpy(l->traj_actions.data(), l->d_traj_actions, sizeof(int32_t) * (size_t)len, hipMemcpyDeviceToHost));
      PLPA3_H(l, hipMemcpy(l->traj_states.data(), l->d_traj_states, sizeof(double) * (size_t)(len + 1) * 13, hipMemcpyDeviceToHost));
    }
  }
  return MPLX_OK;
}

// PlpaArgs of an updateNodes launch
inline void plpa3_update_args(const mplx_plpa3 *l, int32_t world, const mplx::SearchParams &P, mplx::PlpaArgs &A) {
  A = mplx::PlpaArgs{};
  A.st = l->d_st; A.world = world; A.changed = l->d_changed; A.counters = l->d_counters; A.edge_cost = l->d_edge_cost;
  A.succ_child = l->d_succ_child; A.succ_entry = l->d_succ_entry;
  A.changed_cap = (uint32_t)std::min<uint64_t>((uint64_t)P.edge_chunks << mplx::EDGE_CH_LOG, 0xFFFFFFF0ull);
}
inline int plpa3_update_grid(const mplx_plpa3 *l) { return (int)std::min<uint64_t>(1024, (l->st.n_nodes + 63) / 64 + 1); }  // workgroups of a walk over the handle's states
inline void plpa3_changed_sort(mplx_plpa3 *l) {
  std::sort(l->changed.begin(), l->changed.end(), [](uint32_t a, uint32_t b) { return (a & 0x7FFFFFFFu) < (b & 0x7FFFFFFFu); });
}
// after an updateNodes launch, with its counters: the changed entries are fetched (s != nullptr: asynchronously on s; the caller waits
// and calls plpa3_changed_sort)
inline int plpa3_update_finish(mplx_plpa3 *l, const uint32_t ctr[4], uint32_t changed_cap, uint64_t commit_epoch, uint64_t *n_blocked, uint64_t *n_cleared, hipStream_t s) {
  if (ctr[3]) { l->valid = false; return plpa3_fail(&l->err, MPLX_ERR_ARG, "internal: a hyperplane equation of degree > 2 was met by the quadratic-only kernel"); }
  l->synced_epoch = commit_epoch;  // every entry has just been re-tested against the world as committed now
  const uint32_t n = std::min(ctr[2], changed_cap);
  l->changed.resize(n);
  if (s) {
    if (n) PLPA3_H(l, hipMemcpyAsync(l->changed.data(), l->d_changed, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
  } else {
    if (n) PLPA3_H(l, hipMemcpy(l->changed.data(), l->d_changed, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    plpa3_changed_sort(l);
  }
  if (n_blocked) *n_blocked = ctr[0];
  if (n_cleared) *n_cleared = ctr[1];
  return MPLX_OK;
}

// wait for the stream with the poly handle's launch deadline (opt-in, counted from `t0`): past it the abort word of the planner
// context's guard block is raised, which every workgroup of plpa3_plan_kernel polls
inline int plpa3_wait(std::string *err, const mplx_poly3_lpa_view &v, std::chrono::steady_clock::time_point t0, const char *what) {
  using clk = std::chrono::steady_clock;
  bool aborted = false;
  for (;;) {
    const hipError_t e = hipStreamQuery(v.stream);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) return plpa3_fail(err, MPLX_ERR_HIP, "hipStreamQuery failed while waiting for %s: %s", what, hipGetErrorString(e));
    const double el = std::chrono::duration<double>(clk::now() - t0).count();
    if (v.deadline_s > 0 && !aborted && el > v.deadline_s && v.guard) {
      __atomic_store_n(&v.guard->abort, 1u, __ATOMIC_SEQ_CST);
      aborted = true;
    }
    if (aborted && el > v.deadline_s + 10.0) return plpa3_fail(err, MPLX_ERR_TIMEOUT, "%s did not end within %.1f s of its launch and did not answer the abort word", what, v.deadline_s);
    usleep(el < 0.05 ? 50 : 250);
  }
  if (aborted) {
    __atomic_store_n(&v.guard->abort, 0u, __ATOMIC_SEQ_CST);
    return plpa3_fail(err, MPLX_ERR_TIMEOUT, "%s did not end within %.1f s of its launch and was aborted (results of the launch are void)", what, v.deadline_s);
  }
  return MPLX_OK;
}
