// mplx_plpa_space.hip -- the state space of moving-obstacle LPA* planners, exported ON THE DEVICE straight from the handles' pools
// (C-ABI mplx_plpa_export_* / mplx_plpa3_export_*, include/mplx.h): what mplx_plpa_result_nodes / _result_entries decode on the host
// from two pool copies, as passes over the pools (mplx_plpa_space_passes.h) whose results alone cross the bus -- for one handle, or
// for an array of handles bound to one mplx_poly / mplx_poly3 object (a fleet's members) in one launch per pass.  A translation unit
// of its own: the device code of every other unit stays what it is.
//
// The last search / updateNodes launch of every handle has completed before anything here runs (each of those calls waits for its
// launch), and the kernels run on the planner object's stream.  Nothing is cached between calls: a handle's pools change with every
// plan, updateNodes and re-root, so each call runs its pass again.  The scratch buffers belong to the (first) handle and grow on demand.
#include "../../include/mplx.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mplx_poly_lpa_handle.h"
#include "mplx_poly3_lpa_handle.h"
#include "mplx_plpa_space_passes.h"

using namespace mplx;

// One export call = one packed device buffer (a 16-byte header {records kept, error bits}, then one 256-byte-aligned section per
// output the caller asked for), filled by the passes and fetched with ONE copy into pinned host memory, from which the caller's arrays
// are filled -- a handful of runtime calls per export, which is what a read-back of a few hundred states costs.  Above STAGE_MAX
// bytes the sections travel straight into the caller's arrays instead (bandwidth, not call count, decides there).
constexpr size_t STAGE_MAX = 1u << 20;
constexpr size_t PACK_HEADER = 16;

struct PinnedBuf {  // pinned host memory that grows on demand
  char *p = nullptr;
  size_t cap = 0;
  hipError_t need(size_t n) {
    if (n <= cap) return hipSuccess;
    (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t c = 4096;
    while (c < n) c <<= 1;
    hipError_t e = hipHostMalloc((void **)&p, c, hipHostMallocDefault);
    if (e == hipSuccess) cap = c;
    return e;
  }
  void release() { (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct mplx_plpa_space {
  Buf<PlpaSpaceMember> members;
  Buf<char> pack;              // the packed outputs of the call in progress
  Buf<int32_t> child;          // child[entry] of every member, scattered by the nodes pass for the records pass
  Buf<uint32_t> tile_sum, items;
  PinnedBuf up, down;          // descriptors / changed list on their way up, the pack on its way down
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float ms[3] = {0, 0, 0};  // kernel time of the last space / records / changed export
};
void mplx_plpa_space_free(mplx_plpa_space *s) {
  if (!s) return;
  s->members.release(); s->pack.release(); s->child.release(); s->tile_sum.release(); s->items.release(); s->up.release(); s->down.release();
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
}

namespace {

thread_local std::string g_export_error;  // the last refusal of a call that had no handle to keep it in

// the exported row of a 2-D state: pos2 vel2 acc2 jrk2 t out of the pool's pos3 vel3 (acc3) t, as mplx_plpa_result_nodes decodes it
struct Row2 {
  static constexpr int W = 9;
  static __device__ __forceinline__ void decode(const double *st, int nk, double *o) {
    o[0] = st[0]; o[1] = st[1]; o[2] = st[3]; o[3] = st[4];
    o[4] = nk > 6 ? st[6] : 0.0; o[5] = nk > 6 ? st[7] : 0.0;
    o[6] = 0.0; o[7] = 0.0;
    o[8] = st[nk];
  }
};
// of a 3-D state: pos3 vel3 acc3 jrk3 t, as mplx_plpa3_result_nodes decodes it
struct Row3 {
  static constexpr int W = 13;
  static __device__ __forceinline__ void decode(const double *st, int nk, double *o) {
    for (int k = 0; k < 12; k++) o[k] = k < nk ? st[k] : 0.0;
    o[12] = st[nk];
  }
};

struct Dim2 {
  using Handle = mplx_plpa;
  using Row = Row2;
  static constexpr const char *NAME = "mplx_plpa";
  static int stream_of(Handle *l, hipStream_t &s, int &device) {
    mplx_poly_view v;
    if (int r = plpa_poly_view(l->poly, &l->err, v)) return r;
    s = v.stream; device = v.device;
    return MPLX_OK;
  }
};
struct Dim3 {
  using Handle = mplx_plpa3;
  using Row = Row3;
  static constexpr const char *NAME = "mplx_plpa3";
  static int stream_of(Handle *l, hipStream_t &s, int &device) {
    mplx_poly3_lpa_view v;
    if (int r = plpa3_poly_view(l->poly, &l->err, v)) return r;
    s = v.stream; device = v.device;
    return MPLX_OK;
  }
};

template <typename H>
int xfail(H *l, int code, const char *fmt, ...) {
  char buf[768];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (l) l->err = buf;
  g_export_error = buf;
  return code;
}
#define XH(l, x)                                                                                         \
  do {                                                                                                   \
    hipError_t e_ = (x);                                                                                 \
    if (e_ != hipSuccess) return xfail(l, MPLX_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_));     \
  } while (0)

template <typename H>
int pass_err(H *l, uint32_t err) {
  if (err & PERR_LIST) return xfail(l, MPLX_ERR_ARG, "state-space export: corrupt predecessor list");
  if (err & PERR_ENTRY) return xfail(l, MPLX_ERR_ARG, "state-space export: an entry number or a parent id lies outside the state space");
  return xfail(l, MPLX_ERR_ARG, "state-space export: internal: the member descriptors do not cover the tiles");
}

// What an export call works on: the handles' descriptors (a handle without a valid space has none of either kind of tile), the
// stream, the scratch.  Refusals come before any launch.
template <typename D>
struct Work {
  using H = typename D::Handle;
  H *first = nullptr;  // keeps the scratch and the error text
  std::vector<PlpaSpaceMember> m;
  uint64_t n_nodes = 0, n_edges = 0;
  uint32_t node_tiles = 0, edge_tiles = 0;
  hipStream_t stream = nullptr;
  mplx_plpa_space *S = nullptr;

  int open(int32_t n_handles, H *const *l, const char *what, bool upload_members = true) {
    if (n_handles <= 0 || !l) return xfail<H>(nullptr, MPLX_ERR_ARG, "%s: no handles", what);
    for (int32_t i = 0; i < n_handles; i++)
      if (!l[i]) return refuse(n_handles, l, "%s: handle %d is NULL", what, i);
    for (int32_t i = 1; i < n_handles; i++)
      if (l[i]->poly != l[0]->poly) return refuse(n_handles, l, "%s: handle %d is bound to another %s object than handle 0", what, i, D::NAME);
    first = l[0];
    m.resize((size_t)n_handles);
    bool any = false;
    for (int32_t i = 0; i < n_handles; i++) {
      PlpaSpaceMember &M = m[(size_t)i];
      M = PlpaSpaceMember{};
      M.node_tile0 = node_tiles; M.edge_tile0 = edge_tiles;
      M.node_off = n_nodes; M.edge_off = n_edges;
      const H *h = l[i];
      if (!h->valid || !h->node_pool || !h->edge_pool || h->st.n_nodes == 0) continue;
      if (h->pools_valid && ((uint64_t)h->st.n_nodes > (plpa3_chunks_of(h->cap_nodes, NODE_CH_LOG) << NODE_CH_LOG) ||
                             (uint64_t)h->st.n_edges > (plpa3_chunks_of(h->cap_edges, EDGE_CH_LOG) << EDGE_CH_LOG)))
        return refuse(n_handles, l, "%s: handle %d: inconsistent state-space counts", what, i);
      M.node_pool = h->node_pool; M.edge_pool = h->edge_pool;
      M.n_nodes = h->st.n_nodes; M.n_edges = h->st.n_edges;
      M.rb = rec_bytes(h->pool_control); M.hot = rec_hot_bytes(h->pool_control); M.nk = state_len(h->pool_control);
      n_nodes += M.n_nodes; n_edges += M.n_edges;
      node_tiles += (M.n_nodes + TILE - 1) / TILE; edge_tiles += (M.n_edges + TILE - 1) / TILE;
      any = true;
    }
    if (n_edges >= (1ull << 32) || n_nodes >= (1ull << 32)) return refuse(n_handles, l, "%s: more than 2^32 states or entries in one call", what);
    if (!any) return MPLX_OK;
    int device = 0;
    if (int r = D::stream_of(first, stream, device)) return r;
    XH(first, hipSetDevice(device));
    if (!first->space) first->space = new mplx_plpa_space();
    S = first->space;
    if (!S->ev0) { XH(first, hipEventCreate(&S->ev0)); XH(first, hipEventCreate(&S->ev1)); }
    if (upload_members) {
      const size_t mb = sizeof(PlpaSpaceMember) * m.size();
      XH(first, S->members.need(m.size()));
      XH(first, S->up.need(mb));
      memcpy(S->up.p, m.data(), mb);
      XH(first, hipMemcpyAsync(S->members.d, S->up.p, mb, hipMemcpyHostToDevice, stream));
    }
    return MPLX_OK;
  }
  // a refusal that concerns the array: every handle of it carries the text
  int refuse(int32_t n_handles, H *const *l, const char *fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    for (int32_t i = 0; i < n_handles; i++)
      if (l[i]) l[i]->err = buf;
    g_export_error = buf;
    return MPLX_ERR_ARG;
  }
  // the pack of this call: `bytes` of it, header cleared
  int begin(size_t bytes) {
    XH(first, S->pack.need(bytes));
    XH(first, hipMemsetAsync(S->pack.d, 0, PACK_HEADER, stream));
    return MPLX_OK;
  }
  // the first `bytes` of the pack into pinned memory (queued; the caller waits)
  int fetch(size_t bytes) {
    XH(first, S->down.need(bytes));
    XH(first, hipMemcpyAsync(S->down.p, S->pack.d, bytes, hipMemcpyDeviceToHost, stream));
    return MPLX_OK;
  }
  template <typename T>
  T *at(size_t off) const { return (T *)(S->pack.d + off); }
  PlpaSpaceArgs args() const {  // (after begin)
    PlpaSpaceArgs A{};
    A.members = S->members.d; A.n_members = (int32_t)m.size();
    A.node_tiles = node_tiles; A.edge_tiles = edge_tiles;
    A.total = at<unsigned long long>(0); A.err = at<uint32_t>(8);
    return A;
  }
  unsigned long long kept() const { return *(const unsigned long long *)S->down.p; }
  uint32_t err_bits() const { return *(const uint32_t *)(S->down.p + 8); }
};

constexpr size_t PACK_ALIGN = 256;
struct Pack {  // lays the sections of a pack out
  size_t bytes = PACK_ALIGN;  // (the header's section)
  size_t add(bool wanted, size_t n) {
    if (!wanted) return 0;
    const size_t at = bytes;
    bytes += (n + PACK_ALIGN - 1) / PACK_ALIGN * PACK_ALIGN;
    return at;
  }
};

template <typename D>
int export_space(int32_t n_handles, typename D::Handle *const *l, uint64_t cap, uint64_t *offset, double *states, double *g, double *rhs, double *h,
                 int32_t *closed, int32_t *opened, int32_t *built, const char *what) {
  using H = typename D::Handle;
  constexpr int W = D::Row::W;
  if (offset)
    for (int32_t i = 0; i <= n_handles && l; i++) offset[i] = 0;
  Work<D> K;
  if (int r = K.open(n_handles, l, what)) return r;
  if (offset) {
    for (int32_t i = 0; i < n_handles; i++) offset[i] = K.m[(size_t)i].node_off;
    offset[n_handles] = K.n_nodes;
  }
  const size_t n = (size_t)K.n_nodes;
  if (n == 0) return MPLX_OK;
  H *f = K.first;
  if ((uint64_t)n > cap) return xfail(f, MPLX_ERR_CAPACITY, "%s: %zu states, the caller's arrays hold %llu", what, n, (unsigned long long)cap);
  const bool want_flags = closed || opened || built;
  if (!states && !g && !rhs && !h && !want_flags) return MPLX_OK;
  mplx_plpa_space &S = *K.S;
  Pack P;
  const size_t o_states = P.add(states, sizeof(double) * W * n), o_g = P.add(g, sizeof(double) * n), o_rhs = P.add(rhs, sizeof(double) * n),
               o_h = P.add(h, sizeof(double) * n), o_fl = P.add(want_flags, n);
  if (int r = K.begin(P.bytes)) return r;
  PlpaSpaceArgs A = K.args();
  if (states) A.states = K.template at<double>(o_states);
  if (g) A.g = K.template at<double>(o_g);
  if (rhs) A.rhs = K.template at<double>(o_rhs);
  if (h) A.h = K.template at<double>(o_h);
  if (want_flags) A.flags = K.template at<uint8_t>(o_fl);
  hipStream_t s = K.stream;
  XH(f, hipEventRecord(S.ev0, s));
  hipLaunchKernelGGL(plpa_space_nodes_kernel<typename D::Row>, dim3(grid_for(K.node_tiles)), dim3(TILE), 0, s, A);
  XH(f, hipGetLastError());
  XH(f, hipEventRecord(S.ev1, s));
  const bool staged = P.bytes <= STAGE_MAX;
  std::vector<uint8_t> flv;
  if (staged) {
    if (int r = K.fetch(P.bytes)) return r;
  } else {
    if (states) XH(f, hipMemcpyAsync(states, A.states, sizeof(double) * W * n, hipMemcpyDeviceToHost, s));
    if (g) XH(f, hipMemcpyAsync(g, A.g, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (rhs) XH(f, hipMemcpyAsync(rhs, A.rhs, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (h) XH(f, hipMemcpyAsync(h, A.h, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (want_flags) {
      flv.resize(n);
      XH(f, hipMemcpyAsync(flv.data(), A.flags, n, hipMemcpyDeviceToHost, s));
    }
    if (int r = K.fetch(PACK_HEADER)) return r;
  }
  XH(f, hipStreamSynchronize(s));
  XH(f, hipEventElapsedTime(&S.ms[0], S.ev0, S.ev1));
  if (K.err_bits()) return pass_err(f, K.err_bits());
  const char *hp = S.down.p;
  if (staged) {
    if (states) memcpy(states, hp + o_states, sizeof(double) * W * n);
    if (g) memcpy(g, hp + o_g, sizeof(double) * n);
    if (rhs) memcpy(rhs, hp + o_rhs, sizeof(double) * n);
    if (h) memcpy(h, hp + o_h, sizeof(double) * n);
  }
  const uint8_t *fl = staged ? (const uint8_t *)(hp + o_fl) : flv.data();
  if (closed)
    for (size_t i = 0; i < n; i++) closed[i] = (fl[i] & FLAG_CLOSED) ? 1 : 0;
  if (opened)
    for (size_t i = 0; i < n; i++) opened[i] = (fl[i] & FLAG_OPENED) ? 1 : 0;
  if (built)
    for (size_t i = 0; i < n; i++) built[i] = (fl[i] & FLAG_BUILT) ? 1 : 0;
  return MPLX_OK;
}

template <typename D>
int export_records(int32_t n_handles, typename D::Handle *const *l, int32_t which, uint64_t cap, uint64_t *offset, int32_t *entry, int32_t *child, int32_t *parent,
                   int32_t *action, int32_t *blocked, const char *what) {
  using H = typename D::Handle;
  if (offset)
    for (int32_t i = 0; i <= n_handles && l; i++) offset[i] = 0;
  if (which != PLPA_WHICH_ALL && which != PLPA_WHICH_VALID && which != PLPA_WHICH_BLOCKED) {
    for (int32_t i = 0; i < n_handles && l; i++)
      if (l[i]) l[i]->err = "state-space export: which is 0 (all), 1 (valid) or 2 (blocked)";
    return xfail<H>(nullptr, MPLX_ERR_ARG, "%s: which is 0 (all), 1 (valid) or 2 (blocked)", what);
  }
  Work<D> K;
  if (int r = K.open(n_handles, l, what)) return r;
  const size_t ne = (size_t)K.n_edges, nm = K.m.size();
  if (ne == 0) return MPLX_OK;
  H *f = K.first;
  mplx_plpa_space &S = *K.S;
  const bool want_rows = cap > 0 && (entry || child || parent || action || blocked);
  int32_t *const user[5] = {entry, child, parent, action, blocked};
  Pack P;
  const size_t o_first = P.add(true, sizeof(unsigned long long) * nm), head_bytes = P.bytes;
  size_t o_col[5];
  for (int c = 0; c < 5; c++) o_col[c] = P.add(want_rows && user[c], sizeof(int32_t) * ne);
  if (int r = K.begin(P.bytes)) return r;
  PlpaSpaceArgs A = K.args();
  A.which = which;
  A.rec_cap = ne;
  XH(f, S.tile_sum.need(K.edge_tiles));
  A.tile_sum = S.tile_sum.d;
  A.member_first = K.template at<unsigned long long>(o_first);
  int32_t *dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int c = 0; c < 5; c++)
    if (o_col[c]) dev[c] = K.template at<int32_t>(o_col[c]);
  A.r_entry = dev[0]; A.r_child = dev[1]; A.r_parent = dev[2]; A.r_action = dev[3]; A.r_blocked = dev[4];
  hipStream_t s = K.stream;
  if (A.r_child) {
    XH(f, S.child.need(ne));
    XH(f, hipMemsetAsync(S.child.d, 0, sizeof(int32_t) * ne, s));  // (an entry in no list reads 0, as in the host-decoded dump)
    A.child = S.child.d;
  }
  XH(f, hipEventRecord(S.ev0, s));
  if (A.child) hipLaunchKernelGGL(plpa_space_nodes_kernel<typename D::Row>, dim3(grid_for(K.node_tiles)), dim3(TILE), 0, s, A);  // (the child scatter alone)
  hipLaunchKernelGGL(plpa_space_count_kernel, dim3(grid_for(K.edge_tiles)), dim3(TILE), 0, s, A);
  hipLaunchKernelGGL(plpa_space_scan_kernel, dim3(1), dim3(TILE), 0, s, A);
  hipLaunchKernelGGL(plpa_space_write_kernel, dim3(grid_for(K.edge_tiles)), dim3(TILE), 0, s, A);
  XH(f, hipGetLastError());
  XH(f, hipEventRecord(S.ev1, s));
  const bool staged = P.bytes <= STAGE_MAX;
  // straight into the caller's arrays: with no filter the count is known before the passes end, and the rows travel behind them at once
  auto rows_direct = [&](size_t cnt) -> int {
    for (int c = 0; c < 5 && cnt; c++)
      if (dev[c]) XH(f, hipMemcpyAsync(user[c], dev[c], sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, s));
    return MPLX_OK;
  };
  if (int r = K.fetch(staged ? P.bytes : head_bytes)) return r;
  if (!staged && which == PLPA_WHICH_ALL)
    if (int r = rows_direct(cap < (uint64_t)ne ? (size_t)cap : ne)) return r;
  XH(f, hipStreamSynchronize(s));
  XH(f, hipEventElapsedTime(&S.ms[1], S.ev0, S.ev1));
  if (K.err_bits()) return pass_err(f, K.err_bits());
  const size_t total = (size_t)K.kept();
  if (total > ne || (which == PLPA_WHICH_ALL && total != ne)) return xfail(f, MPLX_ERR_ARG, "%s: internal: %zu records kept out of %zu entries", what, total, ne);
  if (offset) {
    const unsigned long long *mf = (const unsigned long long *)(S.down.p + o_first);
    offset[n_handles] = total;
    for (int32_t i = n_handles - 1; i >= 0; i--) offset[i] = K.m[(size_t)i].n_edges ? mf[(size_t)i] : offset[i + 1];
  }
  const size_t cnt = cap < (uint64_t)total ? (size_t)cap : total;
  if (staged) {
    for (int c = 0; c < 5 && cnt; c++)
      if (dev[c]) memcpy(user[c], S.down.p + o_col[c], sizeof(int32_t) * cnt);
  } else if (which != PLPA_WHICH_ALL && want_rows) {
    if (int r = rows_direct(cnt)) return r;
    XH(f, hipStreamSynchronize(s));
  }
  return MPLX_OK;
}

template <typename D>
int export_changed(typename D::Handle *l, uint64_t cap, double *parent_states, int32_t *action, int32_t *now_blocked, uint64_t *n_out, const char *what) {
  using H = typename D::Handle;
  constexpr int W = D::Row::W;
  if (n_out) *n_out = 0;
  H *one[1] = {l};
  Work<D> K;
  if (int r = K.open(1, one, what, false)) return r;
  const size_t n = K.n_nodes ? l->changed.size() : 0;
  if (n_out) *n_out = n;
  const size_t cnt = cap < (uint64_t)n ? (size_t)cap : n;
  if (cnt == 0 || (!parent_states && !action && !now_blocked)) return MPLX_OK;
  mplx_plpa_space &S = *K.S;
  Pack P;
  const size_t o_rows = P.add(parent_states, sizeof(double) * W * cnt), o_action = P.add(action, sizeof(int32_t) * cnt), o_now = P.add(now_blocked, sizeof(int32_t) * cnt);
  if (int r = K.begin(P.bytes)) return r;
  PlpaGatherArgs G{};
  G.m = K.m[0];
  G.n_items = (uint32_t)cnt;
  G.err = K.template at<uint32_t>(8);
  if (parent_states) G.rows = K.template at<double>(o_rows);
  if (action) G.action = K.template at<int32_t>(o_action);
  if (now_blocked) G.now_blocked = K.template at<int32_t>(o_now);
  hipStream_t s = K.stream;
  XH(l, S.items.need(cnt));
  XH(l, S.up.need(sizeof(uint32_t) * cnt));
  memcpy(S.up.p, l->changed.data(), sizeof(uint32_t) * cnt);  // (sorted by entry number: the order of _changed)
  XH(l, hipMemcpyAsync(S.items.d, S.up.p, sizeof(uint32_t) * cnt, hipMemcpyHostToDevice, s));
  G.items = S.items.d;
  XH(l, hipEventRecord(S.ev0, s));
  hipLaunchKernelGGL(plpa_space_gather_kernel<typename D::Row>, dim3(grid_for((cnt + TILE - 1) / TILE)), dim3(TILE), 0, s, G);
  XH(l, hipGetLastError());
  XH(l, hipEventRecord(S.ev1, s));
  const bool staged = P.bytes <= STAGE_MAX;
  if (!staged) {
    if (parent_states) XH(l, hipMemcpyAsync(parent_states, G.rows, sizeof(double) * W * cnt, hipMemcpyDeviceToHost, s));
    if (action) XH(l, hipMemcpyAsync(action, G.action, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, s));
    if (now_blocked) XH(l, hipMemcpyAsync(now_blocked, G.now_blocked, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, s));
  }
  if (int r = K.fetch(staged ? P.bytes : PACK_HEADER)) return r;
  XH(l, hipStreamSynchronize(s));
  XH(l, hipEventElapsedTime(&S.ms[2], S.ev0, S.ev1));
  if (K.err_bits())
    return xfail(l, MPLX_ERR_ARG, "%s: the changed list names entries outside the state space (a new space was planned since the last updateNodes)", what);
  if (staged) {
    if (parent_states) memcpy(parent_states, S.down.p + o_rows, sizeof(double) * W * cnt);
    if (action) memcpy(action, S.down.p + o_action, sizeof(int32_t) * cnt);
    if (now_blocked) memcpy(now_blocked, S.down.p + o_now, sizeof(int32_t) * cnt);
  }
  return MPLX_OK;
}

template <typename H>
int export_ms(const H *l, float ms[3]) {
  if (!l || !ms) return MPLX_ERR_ARG;
  for (int k = 0; k < 3; k++) ms[k] = l->space ? l->space->ms[k] : 0.0f;
  return MPLX_OK;
}

}  // namespace

extern "C" const char *mplx_plpa_export_last_error(void) { return g_export_error.c_str(); }

extern "C" int mplx_plpa_export_space(mplx_plpa *l, uint64_t cap, double *states, double *g, double *rhs, double *h, int32_t *closed, int32_t *opened, int32_t *built,
                                      uint64_t *n) {
  uint64_t off[2] = {0, 0};
  mplx_plpa *one[1] = {l};
  const int r = export_space<Dim2>(1, one, cap, off, states, g, rhs, h, closed, opened, built, "mplx_plpa_export_space");
  if (n) *n = off[1];
  return r;
}
extern "C" int mplx_plpa_export_records(mplx_plpa *l, int32_t which, uint64_t cap, int32_t *entry, int32_t *child, int32_t *parent, int32_t *action, int32_t *blocked,
                                        uint64_t *n) {
  uint64_t off[2] = {0, 0};
  mplx_plpa *one[1] = {l};
  const int r = export_records<Dim2>(1, one, which, cap, off, entry, child, parent, action, blocked, "mplx_plpa_export_records");
  if (n) *n = off[1];
  return r;
}
extern "C" int mplx_plpa_export_changed(mplx_plpa *l, uint64_t cap, double *parent_states, int32_t *action, int32_t *now_blocked, uint64_t *n) {
  return export_changed<Dim2>(l, cap, parent_states, action, now_blocked, n, "mplx_plpa_export_changed");
}
extern "C" int mplx_plpa_export_ms(const mplx_plpa *l, float ms[3]) { return export_ms(l, ms); }
extern "C" int mplx_plpa_export_space_many(int32_t n_handles, mplx_plpa *const *l, uint64_t cap, uint64_t *offset, double *states, double *g, double *rhs, double *h,
                                           int32_t *closed, int32_t *opened, int32_t *built) {
  return export_space<Dim2>(n_handles, l, cap, offset, states, g, rhs, h, closed, opened, built, "mplx_plpa_export_space_many");
}
extern "C" int mplx_plpa_export_records_many(int32_t n_handles, mplx_plpa *const *l, int32_t which, uint64_t cap, uint64_t *offset, int32_t *entry, int32_t *child,
                                             int32_t *parent, int32_t *action, int32_t *blocked) {
  return export_records<Dim2>(n_handles, l, which, cap, offset, entry, child, parent, action, blocked, "mplx_plpa_export_records_many");
}

extern "C" int mplx_plpa3_export_space(mplx_plpa3 *l, uint64_t cap, double *states, double *g, double *rhs, double *h, int32_t *closed, int32_t *opened, int32_t *built,
                                       uint64_t *n) {
  uint64_t off[2] = {0, 0};
  mplx_plpa3 *one[1] = {l};
  const int r = export_space<Dim3>(1, one, cap, off, states, g, rhs, h, closed, opened, built, "mplx_plpa3_export_space");
  if (n) *n = off[1];
  return r;
}
extern "C" int mplx_plpa3_export_records(mplx_plpa3 *l, int32_t which, uint64_t cap, int32_t *entry, int32_t *child, int32_t *parent, int32_t *action, int32_t *blocked,
                                         uint64_t *n) {
  uint64_t off[2] = {0, 0};
  mplx_plpa3 *one[1] = {l};
  const int r = export_records<Dim3>(1, one, which, cap, off, entry, child, parent, action, blocked, "mplx_plpa3_export_records");
  if (n) *n = off[1];
  return r;
}
extern "C" int mplx_plpa3_export_changed(mplx_plpa3 *l, uint64_t cap, double *parent_states, int32_t *action, int32_t *now_blocked, uint64_t *n) {
  return export_changed<Dim3>(l, cap, parent_states, action, now_blocked, n, "mplx_plpa3_export_changed");
}
extern "C" int mplx_plpa3_export_ms(const mplx_plpa3 *l, float ms[3]) { return export_ms(l, ms); }
extern "C" int mplx_plpa3_export_space_many(int32_t n_handles, mplx_plpa3 *const *l, uint64_t cap, uint64_t *offset, double *states, double *g, double *rhs, double *h,
                                            int32_t *closed, int32_t *opened, int32_t *built) {
  return export_space<Dim3>(n_handles, l, cap, offset, states, g, rhs, h, closed, opened, built, "mplx_plpa3_export_space_many");
}
extern "C" int mplx_plpa3_export_records_many(int32_t n_handles, mplx_plpa3 *const *l, int32_t which, uint64_t cap, uint64_t *offset, int32_t *entry, int32_t *child,
                                              int32_t *parent, int32_t *action, int32_t *blocked) {
  return export_records<Dim3>(n_handles, l, which, cap, offset, entry, child, parent, action, blocked, "mplx_plpa3_export_records_many");
}
