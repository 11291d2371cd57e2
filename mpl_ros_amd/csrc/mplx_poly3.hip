// mplx_poly3.hip -- the 3-D moving-obstacle planner (C-ABI mplx_poly3_*, include/mplx.h): PolyMapPlanner<3>'s worlds on the
// device, env_poly_map<3>::get_succ for a batch of states and the device-resident search (mplx_poly3.h).  Its own translation
// unit; the search runs on the pools of an internal planner context (mplx_ctx_ext.h), as the point-cloud planner's does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mplx_ctx_ext.h"
#include "mplx_poly3.h"
#include "mplx_poly3_lpa_host.h"
#include "mplx_poly3_space.h"

using namespace mplx;

static std::string g_poly3_create_error;

struct mplx_poly3 {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool have_cfg = false, committed = false;
  bool any_high_degree = false;  // an obstacle trajectory has a segment above degree two (set by add_nonlinear, cleared by begin)
  int control = 0, n_u = 0;
  double dt = 1, v_max = -1, a_max = -1, j_max = -1, w = 10;
  std::vector<double> U;  // n_u x 3
  double *d_U = nullptr;
  // worlds being assembled on the host
  std::vector<Poly3HP> hps;
  std::vector<Poly3Seg> segs;
  std::vector<Poly3Obs> obs;  // grouped by world at commit
  std::vector<int> obs_world;
  std::vector<Poly3World> worlds;
  // device copies
  Poly3HP *d_hps = nullptr;
  Poly3Seg *d_segs = nullptr;
  Poly3Obs *d_obs = nullptr;
  Poly3World *d_worlds = nullptr;
  int32_t *d_world_of = nullptr;
  int world_cap = 0;
  mplx_ctx *ctx = nullptr;  // pools, batch buffers, guard and result getters of the search
  std::vector<int32_t> last_len;  // trajectory length of every query of the last plan_batch (0: no trajectory)
  // the state-space export (mplx_poly3_space.hip): what the last plan ran with
  uint64_t cfg_epoch = 0, commit_epoch = 0, plan_cfg_epoch = 0, plan_commit_epoch = 0;
  bool plan_general = false;
  std::vector<int32_t> plan_world_of;  // host copy: mplx_poly3_get_succ_batch re-uses d_world_of between the plan and the export
  mplx_poly3_space *space = nullptr;
};

static int p3fail(mplx_poly3 *p, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (p) p->err = buf; else g_poly3_create_error = buf;
  return code;
}
#define P3CHK(p, call)                                                                           \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) return p3fail((p), MPLX_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)
static int from_ctx(mplx_poly3 *p, int r) { return r ? p3fail(p, r, "%s", mplx_ctx_ext_error(p->ctx)) : MPLX_OK; }

extern "C" int mplx_poly3_create(int device, mplx_poly3 **out) {
  if (!out) return p3fail(nullptr, MPLX_ERR_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return p3fail(nullptr, MPLX_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n) return p3fail(nullptr, MPLX_ERR_ARG, "device %d out of range", device);
  mplx_poly3 *p = new mplx_poly3();
  p->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&p->stream) != hipSuccess || mplx_ctx_create(device, &p->ctx) != MPLX_OK) {
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return p3fail(nullptr, MPLX_ERR_HIP, "stream / context creation failed");
  }
  *out = p;
  return MPLX_OK;
}
static void poly3_free_dev(mplx_poly3 *p) {
  (void)hipFree(p->d_hps); (void)hipFree(p->d_segs); (void)hipFree(p->d_obs); (void)hipFree(p->d_worlds);
  p->d_hps = nullptr; p->d_segs = nullptr; p->d_obs = nullptr; p->d_worlds = nullptr;
  p->committed = false;
}
extern "C" void mplx_poly3_destroy(mplx_poly3 *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->stream);
  poly3_free_dev(p);
  mplx_poly3_space_free(p->space);
  p->space = nullptr;
  (void)hipFree(p->d_U);
  (void)hipFree(p->d_world_of);
  mplx_ctx_destroy(p->ctx);
  (void)hipStreamDestroy(p->stream);
  delete p;
}
extern "C" const char *mplx_poly3_last_error(const mplx_poly3 *p) { return p ? p->err.c_str() : g_poly3_create_error.c_str(); }

extern "C" int mplx_poly3_config(mplx_poly3 *p, int32_t control, int32_t n_u, const double *U, double dt, double v_max, double a_max, double j_max, double w) {
  if (!p || !U) return p3fail(p, MPLX_ERR_ARG, "null argument");
  if (control != CTRL_VEL && control != CTRL_ACC && control != CTRL_JRK && control != CTRL_SNP) return p3fail(p, MPLX_ERR_ARG, "control kind %d is not one of VEL / ACC / JRK / SNP", control);
  if (n_u <= 0 || n_u > POLY3_MAX_U) return p3fail(p, MPLX_ERR_ARG, "n_u must be in [1,%d]", POLY3_MAX_U);
  if (!(dt > 0)) return p3fail(p, MPLX_ERR_ARG, "dt must be > 0");
  P3CHK(p, hipSetDevice(p->device));
  p->control = control; p->n_u = n_u; p->dt = dt; p->v_max = v_max; p->a_max = a_max; p->j_max = j_max; p->w = w;
  p->U.assign(U, U + 3 * (size_t)n_u);
  (void)hipFree(p->d_U);
  p->d_U = nullptr;
  P3CHK(p, hipMalloc((void **)&p->d_U, sizeof(double) * 3 * (size_t)n_u));
  P3CHK(p, hipMemcpyAsync(p->d_U, p->U.data(), sizeof(double) * 3 * (size_t)n_u, hipMemcpyHostToDevice, p->stream));
  P3CHK(p, hipStreamSynchronize(p->stream));
  p->have_cfg = true;
  p->cfg_epoch++;
  return MPLX_OK;
}

extern "C" int mplx_poly3_begin(mplx_poly3 *p, int32_t n_worlds) {
  if (!p || n_worlds <= 0) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  p->hps.clear(); p->segs.clear(); p->obs.clear(); p->obs_world.clear();
  p->worlds.assign((size_t)n_worlds, Poly3World());
  p->committed = false;
  p->any_high_degree = false;
  return MPLX_OK;
}
// PolyMapUtil<3>::setBoundingBox (poly_map_util.h:52-68, the -z face's point ori + (dim(0) / 2, dim(2) / 2, 0) included)
// + setStartTime (:21).  Hyperplane3D(ori + q, -e_k) for the lower faces, (ori + dim - q, e_k) for the upper ones.
extern "C" int mplx_poly3_set_world(mplx_poly3 *p, int32_t world, const double ori[3], const double dim[3], double start_t) {
  if (!p || world < 0 || world >= (int)p->worlds.size() || !ori || !dim) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  Poly3World &W = p->worlds[(size_t)world];
  W.start_t = start_t;
  const double h0 = dim[0] / 2, h1 = dim[1] / 2, h2 = dim[2] / 2;
  const double q[6][3] = {{ori[0] + 0.0, ori[1] + h1, ori[2] + h2}, {ori[0] + h0, ori[1] + 0.0, ori[2] + h2}, {ori[0] + h0, ori[1] + h2, ori[2] + 0.0},
                          {(ori[0] + dim[0]) - 0.0, (ori[1] + dim[1]) - h1, (ori[2] + dim[2]) - h2},
                          {(ori[0] + dim[0]) - h0, (ori[1] + dim[1]) - 0.0, (ori[2] + dim[2]) - h2},
                          {(ori[0] + dim[0]) - h0, (ori[1] + dim[1]) - h1, (ori[2] + dim[2]) - 0.0}};
  const double nn[6][3] = {{-1.0, -0.0, -0.0}, {-0.0, -1.0, -0.0}, {-0.0, -0.0, -1.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int k = 0; k < 6; k++)
    for (int a = 0; a < 3; a++) { W.bbox[k].p[a] = q[k][a]; W.bbox[k].n[a] = nn[k][a]; }
  return MPLX_OK;
}
static int poly3_add(mplx_poly3 *p, int32_t world, int kind, int n_hp, const double *hp, Poly3Obs &o) {
  if (!p || world < 0 || world >= (int)p->worlds.size() || n_hp <= 0 || !hp) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  o.kind = kind;
  o.hp_off = (int32_t)p->hps.size();
  o.n_hp = n_hp;
  for (int i = 0; i < n_hp; i++) {
    Poly3HP h;
    for (int a = 0; a < 3; a++) { h.p[a] = hp[6 * i + a]; h.n[a] = hp[6 * i + 3 + a]; }
    p->hps.push_back(h);
  }
  p->obs.push_back(o);
  p->obs_world.push_back(world);
  p->committed = false;
  return MPLX_OK;
}
extern "C" int mplx_poly3_add_static(mplx_poly3 *p, int32_t world, int32_t n_hp, const double *hp, const double pt[3]) {
  Poly3Obs o = Poly3Obs();
  if (pt) for (int a = 0; a < 3; a++) o.p[a] = pt[a];
  return poly3_add(p, world, 0, n_hp, hp, o);
}
extern "C" int mplx_poly3_add_linear(mplx_poly3 *p, int32_t world, int32_t n_hp, const double *hp, const double pt[3], const double v[3], double cov_v) {
  if (!pt || !v) return p3fail(p, MPLX_ERR_ARG, "null argument");
  Poly3Obs o = Poly3Obs();
  for (int a = 0; a < 3; a++) { o.p[a] = pt[a]; o.v[a] = v[a]; }
  o.cov_v = cov_v;
  return poly3_add(p, world, 1, n_hp, hp, o);
}
extern "C" int mplx_poly3_add_nonlinear(mplx_poly3 *p, int32_t world, int32_t n_hp, const double *hp, int32_t n_seg, const double *segs, double start_t, int32_t dis_front,
                                        int32_t dis_back) {
  if (!p || n_seg < 0 || (n_seg > 0 && !segs)) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  if (world < 0 || world >= (int)p->worlds.size() || n_hp <= 0 || !hp) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  Poly3Obs o = Poly3Obs();
  o.seg_off = (int32_t)p->segs.size();
  o.n_seg = n_seg;
  double total = 0.0;
  for (int i = 0; i < n_seg; i++) {
    Poly3Seg s;
    for (int ax = 0; ax < 3; ax++)
      for (int k = 0; k < 6; k++) s.c[ax][k] = segs[19 * i + 6 * ax + k];
    for (int ax = 0; ax < 3; ax++)
      if (s.c[ax][0] != 0 || s.c[ax][1] != 0 || s.c[ax][2] != 0) p->any_high_degree = true;  // (cubic or higher: the general solve())
    s.T = segs[19 * i + 18];
    total = s.T + total;  // Trajectory: taus.push_back(pr.t() + taus.back())
    p->segs.push_back(s);
  }
  o.total_t = total;
  o.start_t = start_t;
  o.dis_front = dis_front ? 1 : 0;
  o.dis_back = dis_back ? 1 : 0;
  return poly3_add(p, world, 2, n_hp, hp, o);
}
extern "C" int mplx_poly3_commit(mplx_poly3 *p) {
  if (!p || p->worlds.empty()) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_begin first");
  P3CHK(p, hipSetDevice(p->device));
  // group the obstacles by world, keeping the order they were added in
  std::vector<Poly3Obs> grouped;
  for (size_t w = 0; w < p->worlds.size(); w++) {
    p->worlds[w].obs_off = (int32_t)grouped.size();
    for (size_t i = 0; i < p->obs.size(); i++)
      if (p->obs_world[i] == (int)w) grouped.push_back(p->obs[i]);
    p->worlds[w].n_obs = (int32_t)grouped.size() - p->worlds[w].obs_off;
  }
  poly3_free_dev(p);
  auto up = [&](auto **d, const auto &v) -> hipError_t {
    using T = typename std::remove_reference<decltype(v)>::type::value_type;
    const size_t bytes = sizeof(T) * (v.size() > 0 ? v.size() : 1);
    hipError_t e = hipMalloc((void **)d, bytes);
    if (e == hipSuccess && !v.empty()) e = hipMemcpyAsync(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, p->stream);
    return e;
  };
  P3CHK(p, up(&p->d_hps, p->hps));
  P3CHK(p, up(&p->d_segs, p->segs));
  P3CHK(p, up(&p->d_obs, grouped));
  P3CHK(p, up(&p->d_worlds, p->worlds));
  P3CHK(p, hipStreamSynchronize(p->stream));
  p->committed = true;
  p->commit_epoch++;
  return MPLX_OK;
}
// hyperplane equations above degree two can occur: JRK / SNP primitives, or an obstacle trajectory with such segments
static bool poly3_general(const mplx_poly3 *p) { return p->control == CTRL_JRK || p->control == CTRL_SNP || p->any_high_degree; }
static Poly3Dev poly3_dev(const mplx_poly3 *p) {
  Poly3Dev D{};
  D.hps = p->d_hps; D.segs = p->d_segs; D.obs = p->d_obs; D.worlds = p->d_worlds;
  D.world_of = p->d_world_of;
  D.U = p->d_U;
  D.control = p->control; D.n_u = p->n_u;
  D.dt = p->dt; D.v_max = p->v_max; D.a_max = p->a_max; D.j_max = p->j_max; D.w = p->w;
  return D;
}
static_assert(sizeof(Poly3SuccOut) == sizeof(mplx_poly3_succ), "Poly3SuccOut must mirror mplx_poly3_succ");
static int ensure_world_of(mplx_poly3 *p, int n) {
  if (p->world_cap >= n) return MPLX_OK;
  (void)hipFree(p->d_world_of);
  p->d_world_of = nullptr;
  p->world_cap = 0;
  P3CHK(p, hipMalloc((void **)&p->d_world_of, sizeof(int32_t) * (size_t)n));
  p->world_cap = n;
  return MPLX_OK;
}

extern "C" int mplx_poly3_get_succ_batch(mplx_poly3 *p, int32_t K, const int32_t *world_of, const double *states, mplx_poly3_succ *out) {
  if (!p || K <= 0 || !world_of || !states || !out) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  if (!p->have_cfg) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_config first");
  if (!p->committed) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_commit first");
  for (int k = 0; k < K; k++)
    if (world_of[k] < 0 || world_of[k] >= (int)p->worlds.size()) return p3fail(p, MPLX_ERR_ARG, "world index out of range");
  P3CHK(p, hipSetDevice(p->device));
  if (int r = ensure_world_of(p, K)) return r;
  double *ds = nullptr;
  Poly3SuccOut *dout = nullptr;
  int32_t *dflags = nullptr;
  const size_t no = (size_t)K * p->n_u;
  auto release = [&]() { (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(dflags); };
  if (hipMalloc((void **)&ds, sizeof(double) * 13 * (size_t)K) != hipSuccess || hipMalloc((void **)&dout, sizeof(Poly3SuccOut) * no) != hipSuccess ||
      hipMalloc((void **)&dflags, sizeof(int32_t)) != hipSuccess) {
    release();
    return p3fail(p, MPLX_ERR_HIP, "get_succ_batch: out of device memory");
  }
  hipError_t e = hipMemcpyAsync(p->d_world_of, world_of, sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, states, sizeof(double) * 13 * (size_t)K, hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(dflags, 0, sizeof(int32_t), p->stream);
  if (e == hipSuccess) {
    const Poly3Dev D = poly3_dev(p);
    const int grid = K < 4096 ? K : 4096;
    if (poly3_general(p))
      hipLaunchKernelGGL((poly3_get_succ_kernel<256, true>), dim3(grid), dim3(256), 0, p->stream, D, (int)K, (const int32_t *)p->d_world_of, (const double *)ds, dout, dflags);
    else
      hipLaunchKernelGGL((poly3_get_succ_kernel<256, false>), dim3(grid), dim3(256), 0, p->stream, D, (int)K, (const int32_t *)p->d_world_of, (const double *)ds, dout, dflags);
    e = hipGetLastError();
  }
  int32_t flags = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(Poly3SuccOut) * no, hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&flags, dflags, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
  release();
  if (e != hipSuccess) return p3fail(p, MPLX_ERR_HIP, "get_succ_batch failed: %s", hipGetErrorString(e));
  if (flags & 1) return p3fail(p, MPLX_ERR_ARG, "internal: a hyperplane equation of degree > 2 was met by the quadratic-only kernel");
  return MPLX_OK;
}

extern "C" int mplx_poly3_set_capacity(mplx_poly3 *p, int32_t n_slots, uint64_t total_nodes, uint64_t total_edges, uint64_t total_open_log) {
  if (!p) return MPLX_ERR_ARG;
  return from_ctx(p, mplx_set_capacity(p->ctx, n_slots, total_nodes, total_edges, total_open_log));
}

template <int CONTROL>
static void launch_search_c(bool general, int grid, hipStream_t s, const SearchParams &P, const Poly3Dev &D) {
  if (general) hipLaunchKernelGGL((astar_poly3_kernel<256, CONTROL, true>), dim3(grid), dim3(256), 0, s, P, D);
  else hipLaunchKernelGGL((astar_poly3_kernel<256, CONTROL, false>), dim3(grid), dim3(256), 0, s, P, D);
}
struct Poly3Launch {
  Poly3Dev dev;
  bool general;
};
static bool launch_search(void *user, int grid, hipStream_t s, const SearchParams &P) {
  const Poly3Launch &L = *(const Poly3Launch *)user;
  switch (P.control) {
    case CTRL_ACC: launch_search_c<CTRL_ACC>(L.general, grid, s, P, L.dev); return true;
    case CTRL_JRK: launch_search_c<CTRL_JRK>(L.general, grid, s, P, L.dev); return true;
    default: return false;
  }
}
// PlannerBase::plan through env_poly_map<3> for n queries in one launch (one workgroup per query): query k plans in world
// world_of[k] from starts[k] (pos3 vel3 acc3 jrk3 t) to goals[k] (same layout; goals carry position, velocity and, for
// JRK, acceleration)
extern "C" int mplx_poly3_plan_batch(mplx_poly3 *p, int32_t n, const int32_t *world_of, const double *starts, const double *goals, double eps, double tol_pos,
                                     double tol_vel, int32_t max_expand, int32_t heur_ignore_dynamics, mplx_result *out) {
  if (!p || n <= 0 || !world_of || !starts || !goals || !out) return p3fail(p, MPLX_ERR_ARG, "bad argument");
  if (!p->have_cfg) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_config first");
  if (!p->committed) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_commit first");
  if (p->control != CTRL_ACC && p->control != CTRL_JRK)
    return p3fail(p, MPLX_ERR_ARG, "the moving-obstacle search runs ACC or JRK states (time-keyed: an SNP state's key would need 13 integers; VEL states have no caller)");
  for (int k = 0; k < n; k++)
    if (world_of[k] < 0 || world_of[k] >= (int)p->worlds.size()) return p3fail(p, MPLX_ERR_ARG, "world index out of range");
  P3CHK(p, hipSetDevice(p->device));
  mplx_config g{};
  g.control = p->control;
  g.n_u = p->n_u;
  g.U = p->U.data();
  g.dt = p->dt; g.v_max = p->v_max; g.a_max = p->a_max; g.j_max = p->j_max; g.w = p->w;
  g.eps = eps;
  g.tol_pos = tol_pos; g.tol_vel = tol_vel; g.tol_acc = -1.0;
  g.t_max = INFINITY;
  g.max_expand = max_expand;
  g.heur_ignore_dynamics = heur_ignore_dynamics;
  g.U_yaw = nullptr; g.yaw_max = 0.0; g.tol_yaw = -1.0;
  if (int r = mplx_planner_config(p->ctx, &g)) return from_ctx(p, r);
  if (int r = ensure_world_of(p, n)) return r;
  P3CHK(p, hipMemcpyAsync(p->d_world_of, world_of, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, p->stream));
  P3CHK(p, hipStreamSynchronize(p->stream));  // (the context's stream launches the search)
  std::vector<QueryIn> in((size_t)n);
  for (int k = 0; k < n; k++) {
    const double *s = starts + 13 * (size_t)k, *gl = goals + 13 * (size_t)k;
    QueryIn &q = in[(size_t)k];
    memset(&q, 0, sizeof(q));
    for (int a = 0; a < 3; a++) {
      q.start.p[a] = s[a]; q.start.v[a] = s[3 + a];
      q.goal.p[a] = gl[a]; q.goal.v[a] = gl[3 + a];
      if (p->control == CTRL_JRK) { q.start.a[a] = s[6 + a]; q.goal.a[a] = gl[6 + a]; }
    }
    q.start_t = s[12];
    q.goal_control = p->control;
  }
  Poly3Launch L{poly3_dev(p), poly3_general(p)};
  p->last_len.clear();
  if (int r = from_ctx(p, mplx_ctx_ext_plan(p->ctx, n, in.data(), launch_search, &L, "the 3-D moving-obstacle search launch", out))) return r;
  p->plan_cfg_epoch = p->cfg_epoch;
  p->plan_commit_epoch = p->commit_epoch;
  p->plan_general = L.general;
  p->plan_world_of.assign(world_of, world_of + n);
  p->last_len.resize((size_t)n);
  for (int k = 0; k < n; k++) p->last_len[(size_t)k] = out[k].status == MPLX_PLAN_OK ? out[k].traj_len : 0;
  for (int k = 0; k < n; k++)
    if (out[k].status == MPLX_PLAN_INTERNAL) return p3fail(p, MPLX_ERR_ARG, "internal: a hyperplane equation of degree > 2 was met by the quadratic-only kernel");
  return MPLX_OK;
}
// trajectory of query q of the last batch: actions[traj_len], node_ids[traj_len + 1], states (traj_len + 1) x 13
extern "C" int mplx_poly3_result_traj(mplx_poly3 *p, int32_t q, int32_t *actions, int32_t *node_ids, double *states) {
  if (!p) return MPLX_ERR_ARG;
  if (q < 0 || q >= (int)p->last_len.size()) return p3fail(p, MPLX_ERR_ARG, "no such query");
  const int len = p->last_len[(size_t)q];
  if (len <= 0) return MPLX_OK;
  std::vector<mplx_waypoint> wps((size_t)len + 1);
  if (int rc = mplx_result_traj(p->ctx, q, nullptr, wps.data(), actions, node_ids)) return from_ctx(p, rc);
  if (states) {
    for (int i = 0; i <= len; i++) {
      double *s = states + 13 * (size_t)i;
      const mplx_waypoint &wp = wps[(size_t)i];
      for (int a = 0; a < 3; a++) { s[a] = wp.pos[a]; s[3 + a] = wp.vel[a]; s[6 + a] = wp.acc[a]; s[9 + a] = 0.0; }
      s[12] = wp.t;
    }
  }
  return MPLX_OK;
}
extern "C" int mplx_poly3_result_nodes(mplx_poly3 *p, int32_t q, uint64_t cap, mplx_waypoint *coords, double *g, int32_t *closed, int32_t *opened) {
  if (!p) return MPLX_ERR_ARG;
  return from_ctx(p, mplx_ctx_ext_nodes(p->ctx, q, cap, coords, g, closed, opened));
}
// (internal: mplx_poly3_space.h) the view the state-space export works with
int mplx_poly3_space_internal_view(mplx_poly3 *p, mplx_poly3_space_view *out) {
  if (!p || !out) return MPLX_ERR_ARG;
  out->dev = poly3_dev(p);
  out->general = p->plan_general ? 1 : 0;
  out->ctx = p->ctx;
  out->plan_world_of = p->plan_world_of.data();
  out->plan_n = (int32_t)p->plan_world_of.size();
  out->commit_epoch = p->commit_epoch; out->plan_commit_epoch = p->plan_commit_epoch;
  out->cfg_epoch = p->cfg_epoch; out->plan_cfg_epoch = p->plan_cfg_epoch;
  out->space = &p->space;
  return MPLX_OK;
}
int mplx_poly3_space_internal_fail(mplx_poly3 *p, int code, const char *msg) { return p3fail(p, code, "%s", msg); }
// (internal: mplx_poly3_lpa_host.h) the view the LPA* works with
int mplx_poly3_lpa_internal_view(mplx_poly3 *p, mplx_poly3_lpa_view *out) {
  if (!p || !out) return MPLX_ERR_ARG;
  if (!p->have_cfg) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_config first");
  if (!p->committed) return p3fail(p, MPLX_ERR_ARG, "mplx_poly3_commit first");
  mplx_ctx_ext_view V;
  if (mplx_ctx_ext_view_get(p->ctx, &V) != MPLX_OK) return p3fail(p, MPLX_ERR_ARG, "internal: no planner context");
  out->dev = poly3_dev(p);
  out->general = poly3_general(p) ? 1 : 0;
  out->n_worlds = (int32_t)p->worlds.size();
  out->device = p->device;
  out->stream = p->stream;
  out->guard = V.guard;
  out->deadline_s = V.deadline_s;
  out->commit_epoch = p->commit_epoch;
  out->cfg_epoch = p->cfg_epoch;
  return MPLX_OK;
}
// plan launches of the handle so far (a wrapper that shares the handle notices that somebody else planned on it since)
extern "C" uint64_t mplx_poly3_plan_epoch(const mplx_poly3 *p) {
  mplx_ctx_ext_view V;
  return p && mplx_ctx_ext_view_get(p->ctx, &V) == MPLX_OK ? V.plan_epoch : 0;
}
extern "C" int mplx_poly3_set_record(mplx_poly3 *p, uint32_t cap) { return p ? from_ctx(p, mplx_set_record(p->ctx, cap)) : MPLX_ERR_ARG; }
extern "C" int mplx_poly3_result_expanded(mplx_poly3 *p, int32_t q, uint32_t cap, int32_t *ids, uint32_t *n) {
  return p ? from_ctx(p, mplx_result_expanded(p->ctx, q, cap, ids, n)) : MPLX_ERR_ARG;
}
extern "C" int mplx_poly3_set_deadline(mplx_poly3 *p, double seconds) { return p ? from_ctx(p, mplx_set_deadline(p->ctx, seconds)) : MPLX_ERR_ARG; }
extern "C" int mplx_poly3_last_kernel_ms(const mplx_poly3 *p, float *ms) { return p ? mplx_last_kernel_ms(p->ctx, ms) : MPLX_ERR_ARG; }
