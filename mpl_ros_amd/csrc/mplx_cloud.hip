// mplx_cloud.hip -- the point-cloud planner (C-ABI mplx_cloud_*, include/mplx.h): EllipsoidPlanner::setMap builds the cloud
// index on the device, env_cloud::get_succ for a batch of states, and the device-resident search (mplx_cloud.h).  Its own
// translation unit; the search runs on the pools of an internal planner context (mplx_ctx_ext.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mplx_cloud.h"
#include "mplx_ctx_ext.h"

using namespace mplx;

static std::string g_cloud_create_error;

struct mplx_cloud {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool have_cfg = false, have_map = false;
  int control = 0, n_u = 0;
  double dt = 1, v_max = -1, a_max = -1, j_max = -1, w = 10;
  std::vector<double> U;  // n_u x 3
  double *d_U = nullptr, *d_ucost = nullptr;
  // the cloud and its index (mplx_cloud.h)
  uint32_t n_pts = 0, n_buckets = 0;
  float4 *d_pf = nullptr;
  double *d_pd = nullptr;
  uint32_t *d_start = nullptr;
  CloudDev dev{};
  unsigned long long *d_tests = nullptr;
  uint64_t last_tests = 0;
  mplx_ctx *ctx = nullptr;  // pools, batch buffers, guard and result getters of the search
  // prior trajectories (P-list of mplx_cloud.h): n_sets tables back to back, p_off[n_sets + 1]; persists until changed
  int n_sets = 0;
  std::vector<int32_t> p_off;
  double *d_p_state = nullptr, *d_p_ctg = nullptr;  // 12 doubles / one double per entry
  int32_t *d_p_ctl = nullptr;
  int32_t *d_p_begin = nullptr, *d_p_count = nullptr;  // per query of the batch being launched
  int p_cap_q = 0;
  int heur_ignore_dynamics = 0;  // of the last mplx_cloud_plan_batch: what mplx_cloud_heuristic_batch uses
};

static int cfail(mplx_cloud *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_cloud_create_error = buf;
  return code;
}
#define CCHK(c, call)                                                                           \
  do {                                                                                          \
    hipError_t e__ = (call);                                                                    \
    if (e__ != hipSuccess) return cfail((c), MPLX_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)
mplx_ctx *mplx_cloud_internal_ctx(mplx_cloud *c) { return c ? c->ctx : nullptr; }
int mplx_cloud_internal_fail(mplx_cloud *c, int code, const char *msg) { return cfail(c, code, "%s", msg); }
static int from_ctx(mplx_cloud *c, int r) { return r ? cfail(c, r, "%s", mplx_ctx_ext_error(c->ctx)) : MPLX_OK; }

extern "C" int mplx_cloud_create(int device, mplx_cloud **out) {
  if (!out) return cfail(nullptr, MPLX_ERR_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return cfail(nullptr, MPLX_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= n) return cfail(nullptr, MPLX_ERR_ARG, "device %d out of range", device);
  mplx_cloud *c = new mplx_cloud();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess || hipMalloc((void **)&c->d_tests, sizeof(unsigned long long)) != hipSuccess ||
      mplx_ctx_create(device, &c->ctx) != MPLX_OK) {
    if (c->d_tests) (void)hipFree(c->d_tests);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return cfail(nullptr, MPLX_ERR_HIP, "stream / context creation failed");
  }
  *out = c;
  return MPLX_OK;
}
static void cloud_free_map(mplx_cloud *c) {
  (void)hipFree(c->d_pf); (void)hipFree(c->d_pd); (void)hipFree(c->d_start);
  c->d_pf = nullptr; c->d_pd = nullptr; c->d_start = nullptr;
  c->have_map = false;
}
static void cloud_free_prior(mplx_cloud *c) {
  (void)hipFree(c->d_p_state); (void)hipFree(c->d_p_ctg); (void)hipFree(c->d_p_ctl);
  c->d_p_state = c->d_p_ctg = nullptr; c->d_p_ctl = nullptr;
  c->n_sets = 0;
  c->p_off.clear();
}
extern "C" void mplx_cloud_destroy(mplx_cloud *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  cloud_free_map(c);
  cloud_free_prior(c);
  (void)hipFree(c->d_p_begin); (void)hipFree(c->d_p_count);
  (void)hipFree(c->d_U); (void)hipFree(c->d_ucost); (void)hipFree(c->d_tests);
  mplx_ctx_destroy(c->ctx);
  (void)hipStreamDestroy(c->stream);
  delete c;
}
extern "C" const char *mplx_cloud_last_error(const mplx_cloud *c) { return c ? c->err.c_str() : g_cloud_create_error.c_str(); }

extern "C" int mplx_cloud_config(mplx_cloud *c, int32_t control, int32_t n_u, const double *U, double dt, double v_max, double a_max, double j_max, double w) {
  if (!c || !U) return cfail(c, MPLX_ERR_ARG, "null argument");
  if (control != CTRL_VEL && control != CTRL_ACC && control != CTRL_JRK && control != CTRL_SNP) return cfail(c, MPLX_ERR_ARG, "control kind %d is not one of VEL / ACC / JRK / SNP", control);
  if (n_u <= 0 || n_u > 256) return cfail(c, MPLX_ERR_ARG, "n_u must be in [1,256]");
  if (!(dt > 0)) return cfail(c, MPLX_ERR_ARG, "dt must be > 0");
  CCHK(c, hipSetDevice(c->device));
  c->control = control; c->n_u = n_u; c->dt = dt; c->v_max = v_max; c->a_max = a_max; c->j_max = j_max; c->w = w;
  c->U.assign(U, U + 3 * (size_t)n_u);
  std::vector<double> ucost((size_t)n_u);  // J(control) + w dt: a function of the control input only (as mplx_planner_config)
  for (int i = 0; i < n_u; i++) {
    double cc[3][6];
    for (int ax = 0; ax < 3; ax++) prim_build_axis(control, 0.0, 0.0, 0.0, 0.0, c->U[3 * i + ax], cc[ax]);
    ucost[(size_t)i] = prim_J(control, cc, dt) + w * dt;
  }
  (void)hipFree(c->d_U); (void)hipFree(c->d_ucost);
  c->d_U = c->d_ucost = nullptr;
  CCHK(c, hipMalloc((void **)&c->d_U, sizeof(double) * 3 * (size_t)n_u));
  CCHK(c, hipMalloc((void **)&c->d_ucost, sizeof(double) * (size_t)n_u));
  CCHK(c, hipMemcpyAsync(c->d_U, c->U.data(), sizeof(double) * 3 * (size_t)n_u, hipMemcpyHostToDevice, c->stream));
  CCHK(c, hipMemcpyAsync(c->d_ucost, ucost.data(), sizeof(double) * (size_t)n_u, hipMemcpyHostToDevice, c->stream));
  CCHK(c, hipStreamSynchronize(c->stream));
  c->have_cfg = true;
  return MPLX_OK;
}

// env_cloud(obs, r, ori, dim): EllipsoidUtil(r) (axe = (r, r, 0.1)), setObstacles (every point: E1), setBoundingBox
extern "C" int mplx_cloud_set_map(mplx_cloud *c, int32_t n, const double *pts, double r, const double ori[3], const double dim[3]) {
  if (!c || n < 0 || (n > 0 && !pts) || !ori || !dim) return cfail(c, MPLX_ERR_ARG, "bad argument");
  if (!(r > 0) || !std::isfinite(r)) return cfail(c, MPLX_ERR_ARG, "the robot radius must be finite and > 0");
  CCHK(c, hipSetDevice(c->device));
  cloud_free_map(c);
  const float rf = (float)r;
  if (!(rf > 0.0f)) return cfail(c, MPLX_ERR_ARG, "the robot radius is below float range");
  uint32_t m = 1;
  while (m < (uint32_t)n) m <<= 1;  // (n < 2^31)
  CloudDev &D = c->dev;
  D = CloudDev{};
  D.n_pts = (uint32_t)n;
  D.bucket_mask = m - 1;
  D.inv_cell = 1.0 / ((double)rf * CLOUD_CELL_MARGIN);
  D.r2f = (float)((double)rf * (double)rf);
  D.axe[0] = r; D.axe[1] = r; D.axe[2] = 0.1;
  // setBoundingBox: Hyperplane3D(point, normal) x 6, in the reference's order and arithmetic
  const double h0 = dim[0] / 2, h1 = dim[1] / 2, h2 = dim[2] / 2;
  const double q[6][3] = {{ori[0] + 0.0, ori[1] + h1, ori[2] + h2}, {ori[0] + h0, ori[1] + 0.0, ori[2] + h2}, {ori[0] + h0, ori[1] + h2, ori[2] + 0.0},
                          {(ori[0] + dim[0]) - 0.0, (ori[1] + dim[1]) - h1, (ori[2] + dim[2]) - h2},
                          {(ori[0] + dim[0]) - h0, (ori[1] + dim[1]) - 0.0, (ori[2] + dim[2]) - h2},
                          {(ori[0] + dim[0]) - h0, (ori[1] + dim[1]) - h1, (ori[2] + dim[2]) - 0.0}};
  const double nn[6][3] = {{-1.0, -0.0, -0.0}, {-0.0, -1.0, -0.0}, {-0.0, -0.0, -1.0}, {1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int k = 0; k < 6; k++)
    for (int a = 0; a < 3; a++) { D.bq[k][a] = q[k][a]; D.bn[k][a] = nn[k][a]; }
  const size_t ns = n > 0 ? (size_t)n : 1;
  CCHK(c, hipMalloc((void **)&c->d_pf, sizeof(float4) * ns));
  CCHK(c, hipMalloc((void **)&c->d_pd, sizeof(double) * 3 * ns));
  CCHK(c, hipMalloc((void **)&c->d_start, sizeof(uint32_t) * ((size_t)m + 1)));
  CCHK(c, hipMemsetAsync(c->d_start, 0, sizeof(uint32_t) * ((size_t)m + 1), c->stream));
  if (n > 0) {  // count, scan, scatter
    double *d_in = nullptr;
    uint32_t *d_bucket = nullptr, *d_count = nullptr;
    auto release = [&]() { (void)hipFree(d_in); (void)hipFree(d_bucket); (void)hipFree(d_count); };
    if (hipMalloc((void **)&d_in, sizeof(double) * 3 * (size_t)n) != hipSuccess || hipMalloc((void **)&d_bucket, sizeof(uint32_t) * (size_t)n) != hipSuccess ||
        hipMalloc((void **)&d_count, sizeof(uint32_t) * (size_t)m) != hipSuccess) {
      release();
      return cfail(c, MPLX_ERR_HIP, "cloud index: out of device memory for %d points", n);
    }
    hipError_t e = hipMemcpyAsync(d_in, pts, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, sizeof(uint32_t) * (size_t)m, c->stream);
    const int g = (int)(((uint32_t)n + 255u) / 256u);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(cloud_index_key_kernel, dim3(g), dim3(256), 0, c->stream, (uint32_t)n, (const double *)d_in, D.inv_cell, D.bucket_mask, d_bucket, d_count);
      hipLaunchKernelGGL(cloud_index_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t *)d_count, m, c->d_start);
      e = hipMemsetAsync(d_count, 0, sizeof(uint32_t) * (size_t)m, c->stream);  // (the scatter's cursors)
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(cloud_index_scatter_kernel, dim3(g), dim3(256), 0, c->stream, (uint32_t)n, (const double *)d_in, (const uint32_t *)d_bucket, (const uint32_t *)c->d_start, d_count, c->d_pf, c->d_pd);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    release();
    if (e != hipSuccess) return cfail(c, MPLX_ERR_HIP, "cloud index build failed: %s", hipGetErrorString(e));
  } else {
    CCHK(c, hipStreamSynchronize(c->stream));
  }
  D.pf = c->d_pf; D.pd = c->d_pd; D.start = c->d_start;
  c->n_pts = (uint32_t)n;
  c->n_buckets = m;
  c->have_map = true;
  return MPLX_OK;
}

static SearchParams succ_params(const mplx_cloud *c) {
  SearchParams P{};
  P.control = c->control;
  P.n_u = c->n_u;
  P.ns = P.nk = key_len_c(c->control);
  P.dt = c->dt; P.v_max = c->v_max; P.a_max = c->a_max; P.j_max = c->j_max; P.w = c->w;
  P.U = c->d_U;
  P.ucost = c->d_ucost;
  return P;
}
static_assert(sizeof(CloudSuccOut) == sizeof(mplx_cloud_succ), "CloudSuccOut must mirror mplx_cloud_succ");

template <int CONTROL>
static void launch_succ(int grid, hipStream_t s, const SearchParams &P, const CloudDev &D, int K, const double *st, CloudSuccOut *o, unsigned long long *t) {
  hipLaunchKernelGGL((cloud_get_succ_kernel<256, CONTROL>), dim3(grid), dim3(256), 0, s, P, D, K, st, o, t);
}
extern "C" int mplx_cloud_get_succ_batch(mplx_cloud *c, int32_t K, const double *states, mplx_cloud_succ *out) {
  if (!c || K <= 0 || !states || !out) return cfail(c, MPLX_ERR_ARG, "bad argument");
  if (!c->have_cfg) return cfail(c, MPLX_ERR_ARG, "mplx_cloud_config first");
  if (!c->have_map) return cfail(c, MPLX_ERR_ARG, "mplx_cloud_set_map first");
  CCHK(c, hipSetDevice(c->device));
  double *ds = nullptr;
  CloudSuccOut *dout = nullptr;
  const size_t no = (size_t)K * c->n_u;
  CCHK(c, hipMalloc((void **)&ds, sizeof(double) * 13 * (size_t)K));
  if (hipMalloc((void **)&dout, sizeof(CloudSuccOut) * no) != hipSuccess) {
    (void)hipFree(ds);
    return cfail(c, MPLX_ERR_HIP, "get_succ_batch: out of device memory");
  }
  hipError_t e = hipMemcpyAsync(ds, states, sizeof(double) * 13 * (size_t)K, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_tests, 0, sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) {
    const SearchParams P = succ_params(c);
    const int grid = K < 4096 ? K : 4096;
    switch (c->control) {
      case CTRL_VEL: launch_succ<CTRL_VEL>(grid, c->stream, P, c->dev, K, ds, dout, c->d_tests); break;
      case CTRL_ACC: launch_succ<CTRL_ACC>(grid, c->stream, P, c->dev, K, ds, dout, c->d_tests); break;
      case CTRL_JRK: launch_succ<CTRL_JRK>(grid, c->stream, P, c->dev, K, ds, dout, c->d_tests); break;
      default: launch_succ<CTRL_SNP>(grid, c->stream, P, c->dev, K, ds, dout, c->d_tests); break;
    }
    e = hipGetLastError();
  }
  unsigned long long tests = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(CloudSuccOut) * no, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&tests, c->d_tests, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(ds);
  (void)hipFree(dout);
  if (e != hipSuccess) return cfail(c, MPLX_ERR_HIP, "get_succ_batch failed: %s", hipGetErrorString(e));
  c->last_tests = tests;
  return MPLX_OK;
}
extern "C" uint64_t mplx_cloud_last_point_tests(const mplx_cloud *c) { return c ? c->last_tests : 0; }

extern "C" int mplx_cloud_set_capacity(mplx_cloud *c, int32_t n_slots, uint64_t total_nodes, uint64_t total_edges, uint64_t total_open_log) {
  if (!c) return MPLX_ERR_ARG;
  return from_ctx(c, mplx_set_capacity(c->ctx, n_slots, total_nodes, total_edges, total_open_log));
}

static void to_state(int control, const double *s, State &o) {
  for (int k = 0; k < 3; k++) {
    o.p[k] = s[k];
    o.v[k] = (control & 2) ? s[3 + k] : 0.0;
    o.a[k] = (control & 4) ? s[6 + k] : 0.0;
    o.j[k] = (control & 8) ? s[9 + k] : 0.0;
  }
}
struct CloudLaunch {
  const CloudDev *dev;
  const CloudPriorDev *prior;  // null: the search without a prior
};
static bool launch_search(void *user, int grid, hipStream_t s, const SearchParams &P) {
  const CloudLaunch &A = *(const CloudLaunch *)user;
  if (A.prior) return mplx_cloud_prior_launch(grid, s, P, *A.dev, *A.prior);
  const CloudDev &D = *A.dev;
  switch (P.control) {
    case CTRL_VEL: hipLaunchKernelGGL((astar_cloud_kernel<256, CTRL_VEL>), dim3(grid), dim3(256), 0, s, P, D); return true;
    case CTRL_ACC: hipLaunchKernelGGL((astar_cloud_kernel<256, CTRL_ACC>), dim3(grid), dim3(256), 0, s, P, D); return true;
    case CTRL_JRK: hipLaunchKernelGGL((astar_cloud_kernel<256, CTRL_JRK>), dim3(grid), dim3(256), 0, s, P, D); return true;
    case CTRL_SNP: hipLaunchKernelGGL((astar_cloud_kernel<256, CTRL_SNP>), dim3(grid), dim3(256), 0, s, P, D); return true;
    default: return false;
  }
}
// n_sets tables of 13-double states (the 13th, t, is not used), control kinds and costs-to-go; see include/mplx.h
extern "C" int mplx_cloud_set_prior(mplx_cloud *c, int32_t n_sets, const int32_t *offsets, const double *states, const int32_t *controls, const double *cost_to_go) {
  if (!c || n_sets < 0) return cfail(c, MPLX_ERR_ARG, "bad argument");
  CCHK(c, hipSetDevice(c->device));
  if (n_sets == 0) {
    cloud_free_prior(c);
    return MPLX_OK;
  }
  if (!offsets || offsets[0] != 0) return cfail(c, MPLX_ERR_ARG, "set_prior: offsets[0] must be 0");
  for (int i = 0; i < n_sets; i++)
    if (offsets[i + 1] < offsets[i]) return cfail(c, MPLX_ERR_ARG, "set_prior: offsets must not decrease (set %d)", i);
  const size_t m = (size_t)offsets[n_sets];
  if (m > 0 && (!states || !controls || !cost_to_go)) return cfail(c, MPLX_ERR_ARG, "set_prior: null table");
  std::vector<double> st(12 * (m ? m : 1));
  for (size_t e = 0; e < m; e++) {
    for (int k = 0; k < 13; k++)
      if (!std::isfinite(states[13 * e + k])) return cfail(c, MPLX_ERR_ARG, "set_prior: entry %zu has a state value that is not finite", e);
    if (!std::isfinite(cost_to_go[e])) return cfail(c, MPLX_ERR_ARG, "set_prior: entry %zu has a cost-to-go that is not finite", e);
    const int k4 = controls[e] & 15;
    if (k4 != CTRL_VEL && k4 != CTRL_ACC && k4 != CTRL_JRK && k4 != CTRL_SNP) return cfail(c, MPLX_ERR_ARG, "set_prior: entry %zu: control kind %d is not one of VEL / ACC / JRK / SNP", e, controls[e]);
    for (int k = 0; k < 12; k++) st[12 * e + k] = states[13 * e + k];
  }
  std::vector<int32_t> ctl(m ? m : 1, 0);
  for (size_t e = 0; e < m; e++) ctl[e] = controls[e] & 15;
  cloud_free_prior(c);
  const size_t ma = m ? m : 1;
  CCHK(c, hipMalloc((void **)&c->d_p_state, sizeof(double) * 12 * ma));
  CCHK(c, hipMalloc((void **)&c->d_p_ctg, sizeof(double) * ma));
  CCHK(c, hipMalloc((void **)&c->d_p_ctl, sizeof(int32_t) * ma));
  if (m > 0) {
    CCHK(c, hipMemcpyAsync(c->d_p_state, st.data(), sizeof(double) * 12 * m, hipMemcpyHostToDevice, c->stream));
    CCHK(c, hipMemcpyAsync(c->d_p_ctg, cost_to_go, sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
    CCHK(c, hipMemcpyAsync(c->d_p_ctl, ctl.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
    CCHK(c, hipStreamSynchronize(c->stream));
  }
  c->p_off.assign(offsets, offsets + n_sets + 1);
  c->n_sets = n_sets;
  return MPLX_OK;
}

extern "C" int mplx_cloud_heuristic_batch(mplx_cloud *c, int32_t K, const double *states, const double *goal, int32_t set, double *h) {
  if (!c || K <= 0 || !states || !goal || !h) return cfail(c, MPLX_ERR_ARG, "bad argument");
  if (!c->have_cfg) return cfail(c, MPLX_ERR_ARG, "mplx_cloud_config first");
  if (set < 0 || set >= (c->n_sets > 0 ? c->n_sets : 1)) return cfail(c, MPLX_ERR_ARG, "heuristic_batch: prior set %d of %d", set, c->n_sets);
  CCHK(c, hipSetDevice(c->device));
  HeurParams hp{};
  hp.w = c->w; hp.v_max = c->v_max; hp.heur_ignore_dynamics = c->heur_ignore_dynamics;
  hp.goal_control = c->control;
  to_state(c->control, goal, hp.goal);
  hp.goal_nkey = state_key(c->control, hp.goal, hp.goal_key);
  CloudPriorView R{nullptr, nullptr, nullptr, 0u};
  if (c->n_sets > 0) {
    const size_t b = (size_t)c->p_off[(size_t)set];
    R = CloudPriorView{c->d_p_state + 12 * b, c->d_p_ctg + b, c->d_p_ctl + b, (uint32_t)(c->p_off[(size_t)set + 1] - c->p_off[(size_t)set])};
  }
  std::vector<double> st(13 * (size_t)K);
  for (int k = 0; k < K; k++) {  // (a state keeps the derivatives its control kind carries, as a query's start does)
    State s;
    to_state(c->control, states + 13 * (size_t)k, s);
    memcpy(&st[13 * (size_t)k], &s, sizeof(double) * 12);
    st[13 * (size_t)k + 12] = states[13 * (size_t)k + 12];
  }
  double *ds = nullptr, *dh = nullptr;
  CCHK(c, hipMalloc((void **)&ds, sizeof(double) * 13 * (size_t)K));
  if (hipMalloc((void **)&dh, sizeof(double) * (size_t)K) != hipSuccess) {
    (void)hipFree(ds);
    return cfail(c, MPLX_ERR_HIP, "heuristic_batch: out of device memory");
  }
  hipError_t e = hipMemcpyAsync(ds, st.data(), sizeof(double) * 13 * (size_t)K, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    mplx_cloud_heuristic_launch(c->stream, c->control, hp, c->dt, R, K, ds, dh);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, dh, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(ds);
  (void)hipFree(dh);
  if (e != hipSuccess) return cfail(c, MPLX_ERR_HIP, "heuristic_batch failed: %s", hipGetErrorString(e));
  return MPLX_OK;
}

extern "C" int mplx_cloud_plan_batch(mplx_cloud *c, int32_t n, const double *starts, const double *goals, double eps, double tol_pos, double tol_vel,
                                     double tol_acc, int32_t max_expand, int32_t heur_ignore_dynamics, mplx_result *out) {
  if (!c || n <= 0 || !starts || !goals || !out) return cfail(c, MPLX_ERR_ARG, "bad argument");
  if (!c->have_cfg) return cfail(c, MPLX_ERR_ARG, "mplx_cloud_config first");
  if (!c->have_map) return cfail(c, MPLX_ERR_ARG, "mplx_cloud_set_map first");
  if (c->n_sets > 1 && c->n_sets != n) return cfail(c, MPLX_ERR_ARG, "plan_batch: %d prior sets are in force for a batch of %d queries (one set, or one per query)", c->n_sets, n);
  c->heur_ignore_dynamics = heur_ignore_dynamics ? 1 : 0;
  mplx_config g{};
  g.control = c->control;
  g.n_u = c->n_u;
  g.U = c->U.data();
  g.dt = c->dt; g.v_max = c->v_max; g.a_max = c->a_max; g.j_max = c->j_max; g.w = c->w;
  g.eps = eps;
  g.tol_pos = tol_pos; g.tol_vel = tol_vel; g.tol_acc = tol_acc;
  g.t_max = INFINITY;
  g.max_expand = max_expand;
  g.heur_ignore_dynamics = heur_ignore_dynamics;
  g.U_yaw = nullptr; g.yaw_max = 0.0; g.tol_yaw = -1.0;
  if (int r = mplx_planner_config(c->ctx, &g)) return from_ctx(c, r);
  std::vector<QueryIn> in((size_t)n);
  for (int k = 0; k < n; k++) {
    QueryIn &q = in[(size_t)k];
    memset(&q, 0, sizeof(q));
    to_state(c->control, starts + 13 * (size_t)k, q.start);
    to_state(c->control, goals + 13 * (size_t)k, q.goal);
    q.start_t = starts[13 * (size_t)k + 12];
    q.goal_control = c->control;
  }
  CloudPriorDev PR{};
  CloudLaunch A{&c->dev, nullptr};
  if (c->n_sets > 0) {  // the batch's own view of the tables: one set for every query, or one per query
    CCHK(c, hipSetDevice(c->device));
    std::vector<int32_t> bc(2 * (size_t)n);
    for (int k = 0; k < n; k++) {
      const size_t s = c->n_sets == 1 ? 0 : (size_t)k;
      bc[(size_t)k] = c->p_off[s];
      bc[(size_t)n + (size_t)k] = c->p_off[s + 1] - c->p_off[s];
    }
    if (n > c->p_cap_q) {
      (void)hipFree(c->d_p_begin); (void)hipFree(c->d_p_count);
      c->d_p_begin = c->d_p_count = nullptr;
      c->p_cap_q = 0;
      CCHK(c, hipMalloc((void **)&c->d_p_begin, sizeof(int32_t) * (size_t)n));
      CCHK(c, hipMalloc((void **)&c->d_p_count, sizeof(int32_t) * (size_t)n));
      c->p_cap_q = n;
    }
    CCHK(c, hipMemcpyAsync(c->d_p_begin, bc.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    CCHK(c, hipMemcpyAsync(c->d_p_count, bc.data() + n, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    CCHK(c, hipStreamSynchronize(c->stream));
    PR = CloudPriorDev{c->d_p_begin, c->d_p_count, c->d_p_state, c->d_p_ctg, c->d_p_ctl};
    A.prior = &PR;
  }
  return from_ctx(c, mplx_ctx_ext_plan(c->ctx, n, in.data(), launch_search, &A, "the point-cloud search launch", out));
}
extern "C" int mplx_cloud_result_traj(mplx_cloud *c, int32_t q, mplx_waypoint *wps, int32_t *actions, int32_t *node_ids) {
  if (!c) return MPLX_ERR_ARG;
  return from_ctx(c, mplx_result_traj(c->ctx, q, nullptr, wps, actions, node_ids));
}
extern "C" int mplx_cloud_result_nodes(mplx_cloud *c, int32_t q, uint64_t cap, mplx_waypoint *coords, double *g, int32_t *closed, int32_t *opened) {
  if (!c) return MPLX_ERR_ARG;
  return from_ctx(c, mplx_ctx_ext_nodes(c->ctx, q, cap, coords, g, closed, opened));
}
extern "C" int mplx_cloud_set_record(mplx_cloud *c, uint32_t cap) { return c ? from_ctx(c, mplx_set_record(c->ctx, cap)) : MPLX_ERR_ARG; }
extern "C" int mplx_cloud_result_expanded(mplx_cloud *c, int32_t q, uint32_t cap, int32_t *ids, uint32_t *n) {
  return c ? from_ctx(c, mplx_result_expanded(c->ctx, q, cap, ids, n)) : MPLX_ERR_ARG;
}
extern "C" int mplx_cloud_set_deadline(mplx_cloud *c, double seconds) { return c ? from_ctx(c, mplx_set_deadline(c->ctx, seconds)) : MPLX_ERR_ARG; }
extern "C" int mplx_cloud_last_kernel_ms(const mplx_cloud *c, float *ms) { return c ? mplx_last_kernel_ms(c->ctx, ms) : MPLX_ERR_ARG; }
