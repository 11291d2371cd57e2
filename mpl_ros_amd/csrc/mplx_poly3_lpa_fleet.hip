// mplx_poly3_lpa_fleet.hip -- C-ABI mplx_plpa3_fleet_* (include/mplx.h): N LPA* planners of the 3-D moving-obstacle environment
// (ordinary mplx_plpa3 handles) on one mplx_poly3 handle whose plan(), updateNodes() and getSubStateSpace() run for all members in ONE
// launch each.  mplx_poly_lpa_fleet.hip one for one, on states of 13 doubles.  The FLEET builds of plpa3_plan_kernel /
// plpa3_update_kernel (mplx_poly3_lpa.h) are instantiated here and nowhere else, so that the single-planner kernels of
// mplx_poly3_lpa.hip are compiled exactly as before; they take what differs between the members from a PlpaMember array (member =
// blockIdx.x for the search, blockIdx.y for the updateNodes walk), the Poly3Dev is the launch's.  A fresh plan runs on the same kernel
// as a repair (PlpaMember::fresh), so fresh plans, repairs and re-roots of different members share a launch.  Per member the host
// decides and books exactly as mplx_plpa3_plan / mplx_plpa3_update_nodes do: through the same functions (mplx_poly3_lpa_handle.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mplx_poly3_lpa_handle.h"

using namespace mplx;

struct mplx_plpa3_fleet {
  mplx_poly3 *poly = nullptr;
  std::string err;
  std::vector<mplx_plpa3 *> m;
  std::vector<int32_t> world_of;
  // one array per kind; the members' LpaState / QueryIn / QueryOut / counters are slices of them
  LpaState *d_st = nullptr;
  QueryIn *d_in = nullptr;
  QueryOut *d_out = nullptr;
  uint32_t *d_counters = nullptr;
  PlpaMember *d_desc = nullptr;
  std::vector<LpaState> h_st;
  std::vector<QueryIn> h_in;
  std::vector<QueryOut> h_out;
  std::vector<uint32_t> h_counters;
  std::vector<PlpaMember> h_desc, h_desc_dev;  // of this launch; what the device holds
  std::vector<int> launched;                   // members of this launch, in descriptor order
  std::vector<Plpa3Query> q;
  uint32_t stats[4] = {0, 0, 0, 0};
  float plan_ms = 0, update_ms = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

static int ff(mplx_plpa3_fleet *f, int code, const char *fmt, ...) {
  char buf[896];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (f) f->err = buf;
  return code;
}
#define FH(f, x)                                                                                      \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) return ff(f, MPLX_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_));     \
  } while (0)

template <bool GEN>
static void launch_fleet_plan(int control, int members, hipStream_t s, const SearchParams &P, const PlpaArgs &A, const Poly3Dev &D) {
  if (control == CTRL_ACC) hipLaunchKernelGGL((plpa3_plan_kernel<CTRL_ACC, GEN, true>), dim3(members), dim3(64), 0, s, P, A, D);
  else hipLaunchKernelGGL((plpa3_plan_kernel<CTRL_JRK, GEN, true>), dim3(members), dim3(64), 0, s, P, A, D);
}
template <bool GEN>
static void launch_fleet_update(int control, int grid_x, int members, hipStream_t s, const SearchParams &P, const PlpaArgs &A, const Poly3Dev &D) {
  if (control == CTRL_ACC) hipLaunchKernelGGL((plpa3_update_kernel<CTRL_ACC, GEN, true>), dim3(grid_x, members), dim3(64), 0, s, P, A, D);
  else hipLaunchKernelGGL((plpa3_update_kernel<CTRL_JRK, GEN, true>), dim3(grid_x, members), dim3(64), 0, s, P, A, D);
}

extern "C" int mplx_plpa3_fleet_create(mplx_poly3 *p, int32_t n, const int32_t *world_of, mplx_plpa3_fleet **out) {
  if (out) *out = nullptr;
  if (!p || !out || !world_of || n < 1 || n > 65535) return MPLX_ERR_ARG;  // (the member is a grid row of the updateNodes launch)
  for (int i = 0; i < n; i++)
    if (world_of[i] < 0) return MPLX_ERR_ARG;
  mplx_plpa3_fleet *f = new mplx_plpa3_fleet();
  f->poly = p;
  for (int i = 0; i < n; i++) {
    mplx_plpa3 *l = nullptr;
    (void)mplx_plpa3_create(p, &l);
    l->in_fleet = true;
    f->m.push_back(l);
    f->world_of.push_back(world_of[i]);
  }
  f->h_st.resize((size_t)n);
  f->h_in.resize((size_t)n);
  f->h_out.resize((size_t)n);
  f->h_counters.resize(4 * (size_t)n);
  f->q.resize((size_t)n);
  *out = f;
  return MPLX_OK;
}
extern "C" void mplx_plpa3_fleet_destroy(mplx_plpa3_fleet *f) {
  if (!f) return;
  mplx_poly3_lpa_view v;
  if (f->d_st && mplx_poly3_lpa_internal_view(f->poly, &v) == MPLX_OK) {
    (void)hipSetDevice(v.device);
    (void)hipStreamSynchronize(v.stream);
  }
  for (mplx_plpa3 *l : f->m) {
    l->in_fleet = false;
    mplx_plpa3_destroy(l);  // (fleet_st set or not: the slices are not the member's to free)
  }
  (void)hipFree(f->d_st); (void)hipFree(f->d_in); (void)hipFree(f->d_out); (void)hipFree(f->d_counters); (void)hipFree(f->d_desc);
  for (hipEvent_t e : f->ev)
    if (e) (void)hipEventDestroy(e);
  delete f;
}
extern "C" const char *mplx_plpa3_fleet_last_error(const mplx_plpa3_fleet *f) { return f ? f->err.c_str() : ""; }
extern "C" int mplx_plpa3_fleet_size(const mplx_plpa3_fleet *f) { return f ? (int)f->m.size() : 0; }
extern "C" mplx_plpa3 *mplx_plpa3_fleet_member(mplx_plpa3_fleet *f, int32_t i) { return f && i >= 0 && (size_t)i < f->m.size() ? f->m[(size_t)i] : nullptr; }
extern "C" int mplx_plpa3_fleet_set_capacity(mplx_plpa3_fleet *f, uint64_t nodes, uint64_t edges, uint64_t open_log) {
  if (!f) return MPLX_ERR_ARG;
  for (mplx_plpa3 *l : f->m) mplx_plpa3_set_capacity(l, nodes, edges, open_log);
  return MPLX_OK;
}
extern "C" int mplx_plpa3_fleet_set_world(mplx_plpa3_fleet *f, int32_t i, int32_t world) {
  if (!f || i < 0 || (size_t)i >= f->m.size() || world < 0) return ff(f, MPLX_ERR_ARG, "member or world index out of range");
  f->world_of[(size_t)i] = world;
  return MPLX_OK;
}
extern "C" int mplx_plpa3_fleet_stats(const mplx_plpa3_fleet *f, uint32_t stats[4]) {
  if (!f || !stats) return MPLX_ERR_ARG;
  memcpy(stats, f->stats, sizeof(f->stats));
  return MPLX_OK;
}
extern "C" int mplx_plpa3_fleet_last_kernel_ms(const mplx_plpa3_fleet *f, float *plan_ms, float *update_ms) {
  if (!f) return MPLX_ERR_ARG;
  if (plan_ms) *plan_ms = f->plan_ms;
  if (update_ms) *update_ms = f->update_ms;
  return MPLX_OK;
}

// the fleet's arrays (first device work of a fleet), the members' slices of them
static int fleet_ensure_arrays(mplx_plpa3_fleet *f, hipStream_t s) {
  if (f->d_st) return MPLX_OK;
  const size_t n = f->m.size();
  FH(f, hipMalloc((void **)&f->d_st, sizeof(LpaState) * n));
  FH(f, hipMalloc((void **)&f->d_in, sizeof(QueryIn) * n));
  FH(f, hipMalloc((void **)&f->d_out, sizeof(QueryOut) * n));
  FH(f, hipMalloc((void **)&f->d_counters, sizeof(uint32_t) * 4 * n));
  FH(f, hipMalloc((void **)&f->d_desc, sizeof(PlpaMember) * n));
  FH(f, hipMemsetAsync(f->d_st, 0, sizeof(LpaState) * n, s));
  FH(f, hipMemsetAsync(f->d_in, 0, sizeof(QueryIn) * n, s));
  FH(f, hipMemsetAsync(f->d_out, 0, sizeof(QueryOut) * n, s));
  for (hipEvent_t &e : f->ev) FH(f, hipEventCreate(&e));
  for (size_t i = 0; i < n; i++) {
    mplx_plpa3 *l = f->m[i];
    if (l->pools_valid) {  // the member was planned on its own (mplx_plpa3_plan) before the fleet's first call: its space moves into the slices
      FH(f, hipMemcpyAsync(f->d_st + i, l->d_st, sizeof(LpaState), hipMemcpyDeviceToDevice, s));
      FH(f, hipStreamSynchronize(s));
      (void)hipFree(l->d_st); (void)hipFree(l->d_in); (void)hipFree(l->d_out); (void)hipFree(l->d_counters);
      l->d_st = f->d_st + i; l->d_in = f->d_in + i; l->d_out = f->d_out + i; l->d_counters = f->d_counters + 4 * i;
    } else if (l->d_st) {  // pools given up by mplx_plpa3_set_capacity: its own four blocks go now (plpa3_free leaves a member's alone)
      (void)hipFree(l->d_st); (void)hipFree(l->d_in); (void)hipFree(l->d_out); (void)hipFree(l->d_counters);
      l->d_st = nullptr; l->d_in = nullptr; l->d_out = nullptr; l->d_counters = nullptr;
    }
    l->fleet_st = f->d_st + i;
    l->fleet_in = f->d_in + i;
    l->fleet_out = f->d_out + i;
    l->fleet_counters = f->d_counters + 4 * i;
  }
  return MPLX_OK;
}
// the poly handle's view; EVERY member's world index must be one of its committed worlds, at each call; a member whose space was
// built before the last mplx_poly3_config drops it, as a single handle does
static int fleet_view(mplx_plpa3_fleet *f, mplx_poly3_lpa_view &v) {
  const int r = plpa3_poly_view(f->poly, &f->err, v);
  if (r) return r;
  for (size_t i = 0; i < f->m.size(); i++)
    if (f->world_of[i] < 0 || f->world_of[i] >= v.n_worlds) return ff(f, MPLX_ERR_ARG, "member %d: world index out of range", (int)i);
  for (mplx_plpa3 *l : f->m) plpa3_config_check(l, v);
  return MPLX_OK;
}
static void fleet_describe(const SearchParams &P, const PlpaArgs &A, PlpaMember &d) {
  d.node_pool = P.node_pool; d.edge_pool = P.edge_pool; d.open_pool = P.open_pool;
  d.table = P.table; d.table_mask = P.table_mask;
  d.bkt_head = P.bkt_head;
  d.st = A.st; d.query = P.queries; d.out = P.out;
  d.traj_nodes = P.traj_nodes; d.traj_actions = P.traj_actions; d.traj_states = P.traj_states;
  d.rec_ids = P.rec_ids;
  d.edge_cost = A.edge_cost; d.succ_child = A.succ_child; d.succ_entry = A.succ_entry;
  d.changed = A.changed; d.counters = A.counters;
  d.node_chunks = P.node_chunks; d.edge_chunks = P.edge_chunks; d.open_chunks = P.open_chunks; d.cap_rec = P.cap_rec;
  d.changed_cap = A.changed_cap;
  d.world = A.world; d.fresh = A.fresh; d.trust_entries = A.trust_entries;
}
// f->h_desc on the device -- copied only when it differs from what the device holds
static int fleet_upload_descriptors(mplx_plpa3_fleet *f, hipStream_t s) {
  const size_t bytes = sizeof(PlpaMember) * f->h_desc.size();
  if (f->h_desc_dev.size() != f->h_desc.size() || memcmp(f->h_desc_dev.data(), f->h_desc.data(), bytes) != 0) {
    f->h_desc_dev = f->h_desc;  // (a copy of its own: the asynchronous upload reads it after h_desc has moved on)
    FH(f, hipMemcpyAsync(f->d_desc, f->h_desc_dev.data(), bytes, hipMemcpyHostToDevice, s));
  }
  return MPLX_OK;
}

// ONE launch of plpa3_plan_kernel for f->launched, whose queries (f->q, f->h_in) are decided; goals: n x 13
static int fleet_launch_plans(mplx_plpa3_fleet *f, const mplx_poly3_lpa_view &v, const double *goals, mplx_result *out) {
  const size_t n = f->m.size();
  hipStream_t s = v.stream;
  SearchParams P{};
  PlpaArgs A{};
  f->h_desc.assign(f->launched.size(), PlpaMember{});
  for (size_t k = 0; k < f->launched.size(); k++) {
    const size_t i = (size_t)f->launched[k];
    mplx_plpa3 *l = f->m[i];
    SearchParams Pm;
    PlpaArgs Am;
    plpa3_params(l, v, Pm);
    plpa3_plan_args(l, v, f->world_of[i], f->q[i].fresh, Am);
    // (the updateNodes fields too: a descriptor that only differs in them would be uploaded again for nothing)
    Am.changed = l->d_changed; Am.counters = l->d_counters;
    Am.changed_cap = (uint32_t)std::min<uint64_t>((uint64_t)Pm.edge_chunks << EDGE_CH_LOG, 0xFFFFFFF0ull);
    if (k == 0) P = Pm;  // (the launch's: the kernel replaces what is a member's)
    fleet_describe(Pm, Am, f->h_desc[k]);
    if (f->q[i].fresh) {
      FH(f, hipMemsetAsync(l->table, 0xFF, (size_t)l->table_slots * sizeof(unsigned long long), s));
      FH(f, hipMemsetAsync(l->d_st, 0, sizeof(LpaState), s));
      f->stats[2]++;
    } else {
      f->stats[0]++;
    }
  }
  FH(f, hipMemcpyAsync(f->d_in, f->h_in.data(), sizeof(QueryIn) * n, hipMemcpyHostToDevice, s));
  int r;
  if ((r = fleet_upload_descriptors(f, s)) != MPLX_OK) return r;
  A.members = f->d_desc;
  FH(f, hipStreamSynchronize(s));  // (the guard block is cleared with no copy in flight, as mplx_plpa3_plan does)
  if (v.guard) memset(v.guard, 0, sizeof(GuardBlock));
  const auto t0 = std::chrono::steady_clock::now();
  FH(f, hipEventRecord(f->ev[0], s));
  if (v.general) launch_fleet_plan<true>(v.dev.control, (int)f->launched.size(), s, P, A, v.dev);
  else launch_fleet_plan<false>(v.dev.control, (int)f->launched.size(), s, P, A, v.dev);
  FH(f, hipGetLastError());
  FH(f, hipEventRecord(f->ev[1], s));
  f->stats[1] = 1;
  if ((r = plpa3_wait(&f->err, v, t0, "the 3-D moving-obstacle LPA* fleet launch")) != MPLX_OK) {
    for (int i : f->launched) {  // aborted: every space of the launch was left in the middle of an expansion
      f->m[(size_t)i]->valid = false;
      f->m[(size_t)i]->traj_len = 0;
    }
    return r;
  }
  FH(f, hipMemcpyAsync(f->h_out.data(), f->d_out, sizeof(QueryOut) * n, hipMemcpyDeviceToHost, s));
  FH(f, hipMemcpyAsync(f->h_st.data(), f->d_st, sizeof(LpaState) * n, hipMemcpyDeviceToHost, s));
  FH(f, hipStreamSynchronize(s));
  FH(f, hipEventElapsedTime(&f->plan_ms, f->ev[0], f->ev[1]));
  int ret = MPLX_OK;
  for (int i : f->launched) {
    mplx_plpa3 *l = f->m[(size_t)i];
    l->last_out = f->h_out[(size_t)i];
    l->st = f->h_st[(size_t)i];
    l->last_ms = f->plan_ms;
    r = plpa3_plan_finish(l, f->q[(size_t)i], v.cfg_epoch, goals + 13 * (size_t)i, out ? &out[i] : nullptr, s);
    if (r != MPLX_OK && ret == MPLX_OK) ret = ff(f, r, "member %d: %s", i, l->err.c_str());  // (that member alone)
  }
  FH(f, hipStreamSynchronize(s));  // (the trajectories)
  return ret;
}

// PlannerBase::plan of every (active) member: the fresh plans and the repairs side by side in one launch
extern "C" int mplx_plpa3_fleet_plan(mplx_plpa3_fleet *f, const double *starts, const double *goals, const int32_t *active, double eps, double tol_pos, double tol_vel,
                                     int32_t max_expand, int32_t heur_ignore_dynamics, mplx_result *out) {
  if (!f || !starts || !goals || !out) return ff(f, MPLX_ERR_ARG, "null argument");
  const int n = (int)f->m.size();
  memset(f->stats, 0, sizeof(f->stats));
  f->plan_ms = 0;
  f->launched.clear();
  for (int i = 0; i < n; i++) {
    memset(&out[i], 0, sizeof(mplx_result));
    if (active && !active[i]) f->stats[3]++;
    else f->launched.push_back(i);
  }
  mplx_poly3_lpa_view v;
  int r = fleet_view(f, v);
  if (r) return r;
  if (f->launched.empty()) return MPLX_OK;
  FH(f, hipSetDevice(v.device));
  if ((r = fleet_ensure_arrays(f, v.stream)) != MPLX_OK) return r;
  for (int i : f->launched) {
    mplx_plpa3 *l = f->m[(size_t)i];
    plpa3_setup(l, eps, tol_pos, tol_vel, max_expand, heur_ignore_dynamics);
    if ((r = plpa3_ensure(l, v.dev.control, v.dev.n_u)) != MPLX_OK) return ff(f, r, "member %d: %s", i, l->err.c_str());
    plpa3_query(l, v.dev.control, starts + 13 * (size_t)i, goals + 13 * (size_t)i, false, f->q[(size_t)i]);
    f->h_in[(size_t)i] = f->q[(size_t)i].in;
  }
  return fleet_launch_plans(f, v, goals, out);
}

// PolyMapPlanner<3>::updateNodes of every member that holds a space, after the worlds were committed again: one launch, member = blockIdx.y
extern "C" int mplx_plpa3_fleet_update_nodes(mplx_plpa3_fleet *f, uint64_t *n_blocked, uint64_t *n_cleared) {
  if (!f) return MPLX_ERR_ARG;
  const size_t n = f->m.size();
  if (n_blocked) memset(n_blocked, 0, sizeof(uint64_t) * n);
  if (n_cleared) memset(n_cleared, 0, sizeof(uint64_t) * n);
  f->update_ms = 0;
  f->launched.clear();
  for (size_t i = 0; i < n; i++) f->m[i]->changed.clear();
  mplx_poly3_lpa_view v;
  int r = fleet_view(f, v);
  if (r) return r;
  for (size_t i = 0; i < n; i++)
    if (f->m[i]->valid) f->launched.push_back((int)i);  // (updateNodes returns at once without a state space: poly_map_planner.h:65)
  if (f->launched.empty()) return MPLX_OK;
  for (int i : f->launched) {
    const mplx_plpa3 *l = f->m[(size_t)i];
    if (!l->pools_valid || l->pool_control != v.dev.control || l->succ_n_u != v.dev.n_u)
      return ff(f, MPLX_ERR_ARG, "member %d: the planner set-up changed since the state space was built", i);
  }
  FH(f, hipSetDevice(v.device));
  hipStream_t s = v.stream;
  if ((r = fleet_ensure_arrays(f, s)) != MPLX_OK) return r;
  SearchParams P{};
  PlpaArgs A{};
  int grid_x = 1;
  f->h_desc.assign(f->launched.size(), PlpaMember{});
  for (size_t k = 0; k < f->launched.size(); k++) {
    const size_t i = (size_t)f->launched[k];
    const mplx_plpa3 *l = f->m[i];
    SearchParams Pm;
    PlpaArgs Am;
    plpa3_params(l, v, Pm);
    plpa3_update_args(l, f->world_of[i], Pm, Am);
    if (k == 0) P = Pm;
    fleet_describe(Pm, Am, f->h_desc[k]);
    grid_x = std::max(grid_x, plpa3_update_grid(l));
  }
  if ((r = fleet_upload_descriptors(f, s)) != MPLX_OK) return r;
  A.members = f->d_desc;
  FH(f, hipMemsetAsync(f->d_counters, 0, sizeof(uint32_t) * 4 * n, s));
  FH(f, hipEventRecord(f->ev[2], s));
  if (v.general) launch_fleet_update<true>(v.dev.control, grid_x, (int)f->launched.size(), s, P, A, v.dev);
  else launch_fleet_update<false>(v.dev.control, grid_x, (int)f->launched.size(), s, P, A, v.dev);
  FH(f, hipGetLastError());
  FH(f, hipEventRecord(f->ev[3], s));
  FH(f, hipMemcpyAsync(f->h_counters.data(), f->d_counters, sizeof(uint32_t) * 4 * n, hipMemcpyDeviceToHost, s));
  FH(f, hipStreamSynchronize(s));
  FH(f, hipEventElapsedTime(&f->update_ms, f->ev[2], f->ev[3]));
  int ret = MPLX_OK;
  for (size_t k = 0; k < f->launched.size(); k++) {
    const size_t i = (size_t)f->launched[k];
    mplx_plpa3 *l = f->m[i];
    r = plpa3_update_finish(l, &f->h_counters[4 * i], f->h_desc[k].changed_cap, v.commit_epoch, n_blocked ? &n_blocked[i] : nullptr, n_cleared ? &n_cleared[i] : nullptr, s);
    if (r != MPLX_OK && ret == MPLX_OK) ret = ff(f, r, "member %d: %s", (int)i, l->err.c_str());  // (that member alone is invalidated)
  }
  FH(f, hipStreamSynchronize(s));  // (the changed lists)
  for (int i : f->launched) plpa3_changed_sort(f->m[(size_t)i]);
  return ret;
}

// PlannerBase::getSubStateSpace(time_step[i]) of member i (< 0: the member is left alone): a fresh plan from the time_step-th state
// of the member's last trajectory to its goal, all members asked in one launch; their stored trajectories are dropped
extern "C" int mplx_plpa3_fleet_sub_state_space(mplx_plpa3_fleet *f, const int32_t *time_step) {
  if (!f || !time_step) return ff(f, MPLX_ERR_ARG, "null argument");
  const size_t n = f->m.size();
  memset(f->stats, 0, sizeof(f->stats));
  f->plan_ms = 0;
  f->launched.clear();
  bool any = false;
  for (size_t i = 0; i < n; i++) any = any || (time_step[i] >= 0 && f->m[i]->valid && f->m[i]->traj_len > 0);
  if (!any) {  // (as mplx_plpa3_sub_state_space without a space or a trajectory: nothing to do, nothing asked of the mplx_poly3 handle)
    f->stats[3] = (uint32_t)n;
    return MPLX_OK;
  }
  mplx_poly3_lpa_view v;
  int r = fleet_view(f, v);
  if (r) return r;
  std::vector<double> starts(13 * n, 0.0), goals(13 * n, 0.0);
  for (size_t i = 0; i < n; i++) {
    const mplx_plpa3 *l = f->m[i];
    if (time_step[i] < 0 || !l->valid || l->traj_len <= 0) {
      f->stats[3]++;
      continue;
    }
    if (time_step[i] > l->traj_len) return ff(f, MPLX_ERR_ARG, "member %d: time_step %d outside the last trajectory (%d primitives)", (int)i, time_step[i], l->traj_len);
    memcpy(&starts[13 * i], &l->traj_states[(size_t)(l->traj_len - time_step[i]) * 13], sizeof(double) * 13);  // (device order is goal -> start)
    for (int k = 0; k < 13; k++) goals[13 * i + k] = l->goal[k];
    f->launched.push_back((int)i);
  }
  if (f->launched.empty()) return MPLX_OK;
  const mplx_plpa3 *l0 = f->m[(size_t)f->launched[0]];
  for (int i : f->launched) {  // (eps, the tolerances, the cap and the heuristic mode are the launch's)
    const mplx_plpa3 *l = f->m[(size_t)i];
    if (l->eps != l0->eps || l->tol_pos != l0->tol_pos || l->tol_vel != l0->tol_vel || l->max_expand != l0->max_expand || l->heur_ignore_dynamics != l0->heur_ignore_dynamics)
      return ff(f, MPLX_ERR_ARG, "member %d was last planned under another set-up (eps / tolerances / cap / heuristic mode) than member %d: re-root it with mplx_plpa3_sub_state_space", i,
                f->launched[0]);
  }
  FH(f, hipSetDevice(v.device));
  if ((r = fleet_ensure_arrays(f, v.stream)) != MPLX_OK) return r;
  for (int i : f->launched) {
    mplx_plpa3 *l = f->m[(size_t)i];
    if ((r = plpa3_ensure(l, v.dev.control, v.dev.n_u)) != MPLX_OK) return ff(f, r, "member %d: %s", i, l->err.c_str());
    plpa3_query(l, v.dev.control, &starts[13 * (size_t)i], &goals[13 * (size_t)i], true, f->q[(size_t)i]);
    f->h_in[(size_t)i] = f->q[(size_t)i].in;
  }
  r = fleet_launch_plans(f, v, goals.data(), nullptr);
  for (int i : f->launched) f->m[(size_t)i]->traj_len = 0;
  return r;
}
