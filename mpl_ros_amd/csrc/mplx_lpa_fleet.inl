// mplx_lpa_fleet.inl -- host side of the LPA* fleets (mplx_lpa_fleet_* of include/mplx.h); included by mplx_api.hip after
// mplx_lpa.inl.  A fleet is N ordinary mplx_lpa planners on one context's map and planner set-up whose repairs and map edits run
// for all members in ONE launch (one per update pass): the FLEET builds of lpa_plan_kernel / lpa_update_kernel
// (mplx_lpa_fleet_launch.hip) take what differs between the members from an LpaMember array.  A member that needs a FRESH plan
// takes mplx_lpa_plan's path, one member after the other, on the ONE import lane the members share.

#include <array>

bool mplx_launch_lpa_fleet(int what, int mode, hipStream_t s, const mplx::SearchParams &P, const mplx::LpaParams &A, int pass, int grid_x, int members);

struct mplx_lpa_fleet {
  mplx_ctx *ctx = nullptr;
  std::string err;
  std::vector<mplx_lpa *> m;
  LpaLane lane;  // the members' import lane
  // one array per kind, the members' LpaState (two spaces each) / QueryIn / QueryOut are slices of them
  LpaState *d_st = nullptr;
  QueryIn *d_in = nullptr;
  QueryOut *d_out = nullptr;
  LpaMember *d_desc = nullptr;
  std::vector<LpaState> h_st;
  std::vector<QueryIn> h_in;
  std::vector<QueryOut> h_out;
  std::vector<LpaMember> h_desc, h_desc_dev;  // of this launch; what the device holds
  std::vector<int> launched;                  // members of this launch, in descriptor order
  uint32_t stats[4] = {0, 0, 0, 0};
  float repair_ms = 0, fresh_ms = 0;
};

static int ffail(mplx_lpa_fleet *f, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (f) f->err = buf;
  return code;
}
#define FCHK(f, call)                                                                                        \
  do {                                                                                                       \
    hipError_t e__ = (call);                                                                                 \
    if (e__ != hipSuccess) return ffail((f), MPLX_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)

extern "C" int mplx_lpa_fleet_create(mplx_ctx *ctx, int32_t n, mplx_lpa_fleet **out) {
  if (!ctx || !out || n < 1 || n > 65535) return MPLX_ERR_ARG;  // (the member is a grid row of the update launches)
  mplx_lpa_fleet *f = new mplx_lpa_fleet();
  f->ctx = ctx;
  for (int i = 0; i < n; i++) {
    mplx_lpa *l = new mplx_lpa();
    l->ctx = ctx;
    l->ln = &f->lane;
    l->fleet = f;
    f->m.push_back(l);
  }
  f->h_st.resize(2 * (size_t)n);
  f->h_in.resize((size_t)n);
  f->h_out.resize((size_t)n);
  *out = f;
  return MPLX_OK;
}
extern "C" void mplx_lpa_fleet_destroy(mplx_lpa_fleet *f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  for (mplx_lpa *l : f->m) {
    l->fleet = nullptr;
    mplx_lpa_destroy(l);  // (fleet_st set or not: the slices are the fleet's)
  }
  lpa_lane_free(&f->lane);
  (void)hipFree(f->d_st); (void)hipFree(f->d_in); (void)hipFree(f->d_out); (void)hipFree(f->d_desc);
  delete f;
}
extern "C" const char *mplx_lpa_fleet_last_error(const mplx_lpa_fleet *f) { return f ? f->err.c_str() : ""; }
extern "C" int mplx_lpa_fleet_size(const mplx_lpa_fleet *f) { return f ? (int)f->m.size() : 0; }
extern "C" mplx_lpa *mplx_lpa_fleet_member(mplx_lpa_fleet *f, int32_t i) { return f && i >= 0 && (size_t)i < f->m.size() ? f->m[(size_t)i] : nullptr; }
extern "C" int mplx_lpa_fleet_set_capacity(mplx_lpa_fleet *f, uint64_t nodes, uint64_t edges, uint64_t open_log) {
  if (!f) return MPLX_ERR_ARG;
  for (mplx_lpa *l : f->m) mplx_lpa_set_capacity(l, nodes, edges, open_log);
  return MPLX_OK;
}
extern "C" int mplx_lpa_fleet_stats(const mplx_lpa_fleet *f, uint32_t stats[4]) {
  if (!f || !stats) return MPLX_ERR_ARG;
  memcpy(stats, f->stats, sizeof(f->stats));
  return MPLX_OK;
}
extern "C" int mplx_lpa_fleet_last_kernel_ms(const mplx_lpa_fleet *f, float *repair_ms, float *fresh_ms) {
  if (!f) return MPLX_ERR_ARG;
  if (repair_ms) *repair_ms = f->repair_ms;
  if (fresh_ms) *fresh_ms = f->fresh_ms;
  return MPLX_OK;
}

// the fleet's arrays (first device work of a fleet), the members' slices of them
static int fleet_ensure_arrays(mplx_lpa_fleet *f) {
  if (f->d_st && f->m[0]->fleet_st) return MPLX_OK;
  const size_t n = f->m.size();
  FCHK(f, hipMalloc((void **)&f->d_st, sizeof(LpaState) * 2 * n));
  FCHK(f, hipMalloc((void **)&f->d_in, sizeof(QueryIn) * n));
  FCHK(f, hipMalloc((void **)&f->d_out, sizeof(QueryOut) * n));
  FCHK(f, hipMalloc((void **)&f->d_desc, sizeof(LpaMember) * n));
  FCHK(f, hipMemsetAsync(f->d_st, 0, sizeof(LpaState) * 2 * n, f->ctx->stream));
  FCHK(f, hipMemsetAsync(f->d_in, 0, sizeof(QueryIn) * n, f->ctx->stream));
  for (size_t i = 0; i < n; i++) {
    f->m[i]->fleet_st = f->d_st + 2 * i;
    f->m[i]->fleet_in = f->d_in + i;
    f->m[i]->fleet_out = f->d_out + i;
  }
  return MPLX_OK;
}

static int fleet_ensure(mplx_lpa_fleet *f, std::string *why) {
  const int r = fleet_ensure_arrays(f);
  if (r != MPLX_OK && why) *why = f->err;
  return r;
}

// the descriptors of f->launched (current spaces) on the device -- copied only when they differ from what it holds; P: the
// launch's SearchParams (the first member's: the kernels replace what is a member's), A.members set
static int fleet_descriptors(mplx_lpa_fleet *f, SearchParams &P, LpaParams &A) {
  f->h_desc.assign(f->launched.size(), LpaMember{});
  for (size_t k = 0; k < f->launched.size(); k++) {
    const mplx_lpa *l = f->m[(size_t)f->launched[k]];
    SearchParams Pm;
    LpaParams Am;
    lpa_params(l, l->cur, Pm, Am);
    if (k == 0) { P = Pm; A = Am; }
    LpaMember &d = f->h_desc[k];
    d.node_pool = Pm.node_pool; d.edge_pool = Pm.edge_pool; d.open_pool = Pm.open_pool;
    d.table = Pm.table; d.table_mask = Pm.table_mask;
    d.bkt_head = Pm.bkt_head;
    d.st = Am.st; d.blocked_log = Am.blocked_log;
    d.query = Pm.queries; d.out = Pm.out;
    d.traj_nodes = Pm.traj_nodes; d.traj_actions = Pm.traj_actions; d.traj_states = Pm.traj_states;
    d.rec_ids = Pm.rec_ids;
    d.node_chunks = Pm.node_chunks; d.edge_chunks = Pm.edge_chunks; d.open_chunks = Pm.open_chunks;
    d.cap_rec = Pm.cap_rec; d.blocked_cap = Am.blocked_cap;
  }
  const size_t bytes = sizeof(LpaMember) * f->h_desc.size();
  if (f->h_desc_dev.size() != f->h_desc.size() || memcmp(f->h_desc_dev.data(), f->h_desc.data(), bytes) != 0) {
    f->h_desc_dev = f->h_desc;  // (a copy of its own: the asynchronous upload reads it after h_desc has moved on)
    FCHK(f, hipMemcpyAsync(f->d_desc, f->h_desc_dev.data(), bytes, hipMemcpyHostToDevice, f->ctx->stream));
  }
  A.fresh = 0;
  A.members = f->d_desc;
  return MPLX_OK;
}

// PlannerBase::plan of every (active) member.  Decides per member as mplx_lpa_plan does; the repairs share one launch.
extern "C" int mplx_lpa_fleet_plan(mplx_lpa_fleet *f, const mplx_waypoint *starts, const mplx_waypoint *goals, const int32_t *active, mplx_result *out) {
  if (!f || !starts || !goals || !out) return ffail(f, MPLX_ERR_ARG, "null argument");
  mplx_ctx *c = f->ctx;
  const int n = (int)f->m.size();
  int r;
  for (int i = 0; i < n; i++) {
    if (active && !active[i]) continue;
    if (const char *why = lpa_plan_refusal(c, &starts[i], &goals[i], &r)) return ffail(f, r, "member %d: %s", i, why);
  }
  if (c->cfg.n_u > 128) return ffail(f, MPLX_ERR_ARG, "LPA* supports lattices of at most 128 control inputs (got %d)", c->cfg.n_u);
  FCHK(f, hipSetDevice(c->device));
  if ((r = fleet_ensure(f, nullptr)) != MPLX_OK) return r;
  memset(f->stats, 0, sizeof(f->stats));
  f->repair_ms = f->fresh_ms = 0;
  f->launched.clear();
  std::vector<int> fresh_members;
  std::vector<std::array<int32_t, MAX_KEY>> keys((size_t)n);
  for (int i = 0; i < n; i++) {
    memset(&out[i], 0, sizeof(mplx_result));
    if (active && !active[i]) {
      f->stats[3]++;
      continue;
    }
    mplx_lpa *l = f->m[(size_t)i];
    if ((r = lpa_ensure(l)) != MPLX_OK) return ffail(f, r, "member %d: %s", i, l->err.c_str());
    keys[(size_t)i].fill(0);
    f->h_in[(size_t)i] = QueryIn{};
    if (lpa_query(l, &starts[i], &goals[i], f->h_in[(size_t)i], keys[(size_t)i].data())) fresh_members.push_back(i);
    else f->launched.push_back(i);
  }
  // ---- the repairs: one upload of the queries, one launch, one download of the results and of the spaces' scalars
  // (every active member's query: the map updates read the goal of a member's last plan from its slice)
  if (f->stats[3] < (uint32_t)n) FCHK(f, hipMemcpyAsync(f->d_in, f->h_in.data(), sizeof(QueryIn) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  if (!f->launched.empty()) {
    SearchParams P;
    LpaParams A;
    if ((r = fleet_descriptors(f, P, A)) != MPLX_OK) return r;
    guard_arm(c);
    FCHK(f, hipEventRecord(c->ev0, c->stream));
    if (!mplx_launch_lpa_fleet(0, 0, c->stream, P, A, 0, 1, (int)f->launched.size())) return ffail(f, MPLX_ERR_ARG, "lattice too wide for LPA*");
    FCHK(f, hipGetLastError());
    FCHK(f, hipEventRecord(c->ev1, c->stream));
    if (int rw = guard_wait(c, c->stream, "the LPA* fleet launch")) {  // aborted: every space of the launch was left in the middle of an expansion
      for (int i : f->launched) {
        f->m[(size_t)i]->valid = false;
        f->m[(size_t)i]->traj_len = 0;
      }
      return ffail(f, rw, "%s", c->err.c_str());
    }
    FCHK(f, hipMemcpyAsync(f->h_out.data(), f->d_out, sizeof(QueryOut) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FCHK(f, hipMemcpyAsync(f->h_st.data(), f->d_st, sizeof(LpaState) * 2 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    FCHK(f, hipStreamSynchronize(c->stream));
    FCHK(f, hipEventElapsedTime(&f->repair_ms, c->ev0, c->ev1));
    for (int i : f->launched) {
      mplx_lpa *l = f->m[(size_t)i];
      l->last_out = f->h_out[(size_t)i];
      l->st = f->h_st[2 * (size_t)i + (size_t)l->cur];
      l->last_ms = f->repair_ms;
      if ((r = lpa_plan_finish(l, false, keys[(size_t)i].data(), &goals[i], &out[i], false)) != MPLX_OK) return ffail(f, r, "member %d: %s", i, l->err.c_str());
    }
    FCHK(f, hipStreamSynchronize(c->stream));  // (the trajectories)
    f->stats[0] = (uint32_t)f->launched.size();
    f->stats[1] = 1;
  }
  // ---- the fresh plans: mplx_lpa_plan's path on the shared lane, one member after the other
  for (int i : fresh_members) {
    mplx_lpa *l = f->m[(size_t)i];
    if ((r = mplx_lpa_plan(l, &starts[i], &goals[i], &out[i])) != MPLX_OK) return ffail(f, r, "member %d: %s", i, l->err.c_str());
    f->fresh_ms += l->last_ms;
    f->stats[2]++;
  }
  return MPLX_OK;
}

// MapPlanner::updateBlockedNodes / updateClearedNodes of every member that holds a space, after the context's map was edited: the
// three passes of lpa_update, each ONE launch with the member in blockIdx.y
static int fleet_update(mplx_lpa_fleet *f, int mode, int n_cells, const int32_t *cells, uint64_t *n_changed) {
  if (!f || n_cells < 0 || (n_cells > 0 && !cells)) return ffail(f, MPLX_ERR_ARG, "bad argument");
  mplx_ctx *c = f->ctx;
  const size_t n = f->m.size();
  if (n_changed) memset(n_changed, 0, sizeof(uint64_t) * n);
  f->launched.clear();
  for (size_t i = 0; i < n; i++)
    if (f->m[i]->valid) f->launched.push_back((int)i);
  if (f->launched.empty() || n_cells == 0) return MPLX_OK;
  for (int i : f->launched)
    if (!lpa_same_setup(f->m[(size_t)i])) return ffail(f, MPLX_ERR_ARG, "the planner set-up on the context changed since the LPA* state space of member %d was built", i);
  FCHK(f, hipSetDevice(c->device));
  SearchParams P;
  LpaParams A;
  int r;
  if ((r = fleet_descriptors(f, P, A)) != MPLX_OK) return r;
  // (n_changed of every space of the fleet: one strided fill)
  FCHK(f, hipMemset2DAsync(&f->d_st->n_changed, sizeof(LpaState), 0, sizeof(unsigned long long), 2 * n, c->stream));
  const int members = (int)f->launched.size();
  const int wide = std::max(1, 4 * c->n_cus / members);  // the machine's worth of workgroups, shared between the members
  if (!mplx_launch_lpa_fleet(1, mode, c->stream, P, A, 0, wide, members)) return ffail(f, MPLX_ERR_ARG, "lattice too wide for LPA*");
  if (mode == 1) mplx_launch_lpa_fleet(1, mode, c->stream, P, A, 1, 1, members);
  mplx_launch_lpa_fleet(1, mode, c->stream, P, A, 2, wide, members);
  FCHK(f, hipGetLastError());
  FCHK(f, hipMemcpyAsync(f->h_st.data(), f->d_st, sizeof(LpaState) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  FCHK(f, hipStreamSynchronize(c->stream));
  int ret = MPLX_OK;
  for (int i : f->launched) {
    mplx_lpa *l = f->m[(size_t)i];
    l->st = f->h_st[2 * (size_t)i + (size_t)l->cur];
    if (l->st.n_changed == ~0ull) {  // this member's conversion ran out of pool: it is dropped alone
      l->valid = false;
      (void)lfail(l, MPLX_ERR_CAPACITY, "LPA* pools exhausted while turning cleared primitives into predecessor entries (mplx_lpa_set_capacity)");
      ret = ffail(f, MPLX_ERR_CAPACITY, "member %d: %s", i, l->err.c_str());
    }
    if (n_changed) n_changed[i] = l->st.n_changed;
  }
  return ret;
}
extern "C" int mplx_lpa_fleet_update_blocked(mplx_lpa_fleet *f, int n_cells, const int32_t *cells, uint64_t *n_changed) { return fleet_update(f, 0, n_cells, cells, n_changed); }
extern "C" int mplx_lpa_fleet_update_cleared(mplx_lpa_fleet *f, int n_cells, const int32_t *cells, uint64_t *n_changed) { return fleet_update(f, 1, n_cells, cells, n_changed); }

// PlannerBase::getSubStateSpace(time_step[i]) of member i, one member after the other (< 0: the member is left alone)
extern "C" int mplx_lpa_fleet_sub_state_space(mplx_lpa_fleet *f, const int32_t *time_step) {
  if (!f || !time_step) return ffail(f, MPLX_ERR_ARG, "null argument");
  int ret = MPLX_OK;
  for (size_t i = 0; i < f->m.size(); i++) {
    if (time_step[i] < 0) continue;
    const int r = mplx_lpa_sub_state_space(f->m[i], time_step[i]);
    if (r != MPLX_OK && ret == MPLX_OK) ret = ffail(f, r, "member %d: %s", (int)i, f->m[i]->err.c_str());
  }
  return ret;
}
